#!/usr/bin/env python3
"""Time of the doc-set filtered calls (wsr_search_bool_filtered,
wsr_count_bool_filtered, wsr_docset_from_bool) on the C3 stand-in, beside the
unfiltered wsr_search_bool and wsr_count_bool on the same queries.

The workload is count_bench.py's: the first --queries queries of the two-term
log that `bench.py --prepare` writes, k = 10, in three role forms; per form and
per entry point a warm-up call, then --calls timed calls.  In one session, per
form: the unfiltered search and count; the filtered calls with the set of all
docs (the filter's overhead, a measured number with no bar set in advance); the
filtered calls with a range of one sixteenth of the doc ids; and
wsr_docset_from_bool, one call per query.
The condition, without a margin, per form, for search and for count: the
range-filtered median is no more than the fastest of the unfiltered calls -- it
does a subset of the same work.
Also checked: the full-set answers equal the unfiltered ones (hits and
counts), and every range-filtered count equals the number of ids inside the
range that wsr_docset_ids gives for the query's match set.
Writes one JSON object (--out, default profiles/docset/bench.json), prints it,
and exits 1 when a condition fails.
"""
import argparse
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--index-dir", default=None, help="the C3 stand-in (default: found under bench.py's index dir)")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--queries", type=int, default=4096)
    p.add_argument("--calls", type=int, default=9)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "docset", "bench.json"))
    a = p.parse_args()

    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process, as bench.py)
    import bench
    import wiser_amd as w
    from wiser_amd import _capi
    lib = _capi.lib
    idx = a.index_dir
    if not idx:
        found = sorted(glob.glob(os.path.join(bench.default_index_dir(), "c3_wiki_*", "READY")))
        if not found:
            raise SystemExit("no C3 stand-in: run `python bench.py --prepare` first")
        idx = os.path.dirname(found[0])
    log = os.path.join(idx, "two_term_100000.log")
    items = [t for t, ph in w.read_query_log(log) if not ph][:a.queries]
    n = len(items)
    eng = w.VacuumEngine(idx, positions=False)
    eng.Load()
    n_docs = eng.NumDocs()
    lo = (n_docs // 2) + 1000          # (a range that begins and ends inside a window)
    hi = lo + n_docs // 16
    full, rng = eng.docset(np.arange(n_docs, dtype=np.int32)), eng.docset(np.arange(lo, hi, dtype=np.int32))
    f_full = (C.c_void_p * n)(*([full._s] * n))
    f_rng = (C.c_void_p * n)(*([rng._s] * n))

    def timed(step):
        step()   # warm-up: the context's buffers grow here
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            step()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def stats_of(st):
        return {"items": st.items, "windows": st.windows, "windows_skipped": st.windows_skipped,
                "touched_docs": st.touched_docs, "events": st.events}

    def row(ts, st):
        return {"median_ms": round(statistics.median(ts), 3), "fastest_ms": round(min(ts), 3),
                "calls_ms": [round(x, 3) for x in ts], "stats": stats_of(st)}

    out = {"workload": "c3_two_term_docset", "index": os.path.basename(idx), "k": a.k, "queries": n,
           "calls": a.calls, "n_docs": n_docs, "range": [lo, hi], "forms": {}}
    ok = True
    for form, roles in (("must_must", ("must", "must")), ("must_should", ("must", "should")),
                        ("should_should", ("should", "should"))):
        arr = (_capi.BoolQuery * n)(*[eng.resolve_bool(w.BoolQuery(list(zip(t, roles)), n_results=a.k))[0]
                                      for t in items])

        def search(filters):
            hits, nh, st = (_capi.Hit * (n * a.k))(), (C.c_int32 * n)(), _capi.OrStats()

            def step():
                if filters is None:
                    _capi.check(lib.wsr_search_bool_ex(eng._h, arr, n, a.k, hits, nh, 0, C.byref(st)))
                else:
                    _capi.check(lib.wsr_search_bool_filtered(eng._h, arr, n, filters, a.k, hits, nh, 0, C.byref(st)))
            ts = timed(step)
            got = [[(hits[i * a.k + j].doc_id, hits[i * a.k + j].score) for j in range(nh[i])] for i in range(n)]
            return ts, st, got

        def count(filters):
            counts, st = (C.c_int64 * n)(), _capi.OrStats()

            def step():
                if filters is None:
                    _capi.check(lib.wsr_count_bool_ex(eng._h, arr, n, counts, 0, C.byref(st)))
                else:
                    _capi.check(lib.wsr_count_bool_filtered(eng._h, arr, n, filters, counts, 0, C.byref(st)))
            ts = timed(step)
            return ts, st, list(counts)

        s_ts, s_st, s_got = search(None)
        c_ts, c_st, c_got = count(None)
        sf_ts, sf_st, sf_got = search(f_full)
        cf_ts, cf_st, cf_got = count(f_full)
        sr_ts, sr_st, sr_got = search(f_rng)
        cr_ts, cr_st, cr_got = count(f_rng)
        # wsr_docset_from_bool, one call per query; the ids of each set inside the range
        in_range, set_sizes, fb_ms = [], [], []
        for i in range(n):
            s = C.c_void_p()
            t0 = time.perf_counter()
            _capi.check(lib.wsr_docset_from_bool(eng._h, C.byref(arr[i]), None, 0, C.byref(s)))
            fb_ms.append((time.perf_counter() - t0) * 1e3)
            ds = w.DocSet(eng, s)
            ids = ds.ids()
            ds.close()
            set_sizes.append(int(ids.size))
            in_range.append(int(np.count_nonzero((ids >= lo) & (ids < hi))))
        bad_full = sum(1 for x, y in zip(s_got, sf_got) if x != y) + sum(1 for x, y in zip(c_got, cf_got) if x != y)
        bad_sets = sum(1 for x, y in zip(c_got, set_sizes) if x != y)
        bad_range = sum(1 for x, y in zip(cr_got, in_range) if x != y)
        bad_hits = sum(1 for g, c in zip(sr_got, cr_got)
                       if len(g) != min(a.k, c) or any(not lo <= d < hi for d, _ in g))
        s_holds = statistics.median(sr_ts) <= min(s_ts)
        c_holds = statistics.median(cr_ts) <= min(c_ts)
        ok = ok and s_holds and c_holds and not (bad_full or bad_sets or bad_range or bad_hits)
        out["forms"][form] = {
            "search_bool": row(s_ts, s_st), "count_bool": row(c_ts, c_st),
            "search_full_set": row(sf_ts, sf_st), "count_full_set": row(cf_ts, cf_st),
            "search_range": row(sr_ts, sr_st), "count_range": row(cr_ts, cr_st),
            "from_bool_per_query": {"median_ms": round(statistics.median(fb_ms), 4),
                                    "mean_ms": round(sum(fb_ms) / n, 4), "total_ms": round(sum(fb_ms), 1)},
            "matches": sum(c_got), "matches_in_range": sum(cr_got),
            "search_range_median_at_most_fastest_unfiltered": s_holds,
            "count_range_median_at_most_fastest_unfiltered": c_holds,
            "mismatches_full_set": bad_full, "mismatches_match_set_size": bad_sets,
            "mismatches_range_count": bad_range, "mismatches_range_hits": bad_hits}
        print(f"[docset_bench] {form}: search {statistics.median(s_ts):.3f} / full {statistics.median(sf_ts):.3f} / "
              f"range {statistics.median(sr_ts):.3f} ms; count {statistics.median(c_ts):.3f} / "
              f"full {statistics.median(cf_ts):.3f} / range {statistics.median(cr_ts):.3f} ms",
              file=sys.stderr, flush=True)
    out["mismatches"] = sum(v[k] for v in out["forms"].values() for k in v if k.startswith("mismatches_"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    full.close()
    rng.close()
    eng.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
