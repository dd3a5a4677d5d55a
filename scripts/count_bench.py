#!/usr/bin/env python3
"""Time of exact match counts (wsr_count_bool) on the C3 stand-in, beside
wsr_search_bool at k = 10 on the same queries.

Runs the first --queries queries of the two-term log that `bench.py --prepare`
writes under $WISER_BENCH_DIR (or bench.py's default index directory) in three
forms: both terms MUST, the first MUST and the second SHOULD, both SHOULD.  Per
form and per entry point: a warm-up call, then --calls timed calls (a call is
synchronous: copies in, kernel(s), copies out, one wait).  The condition, per
form: the count call's median is no more than the fastest wsr_search_bool call
-- counting does a subset of that call's work.  Also checked: the count is at
least wsr_search_bool's n_hits, equal when it is at most k, and the two-term
identities count(a b) = df(a) + df(b) - count(+a +b).
Writes one JSON object (--out, default profiles/count/bench.json), prints it,
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "count", "bench.json"))
    a = p.parse_args()

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

    out = {"workload": "c3_two_term_count", "index": os.path.basename(idx), "k": a.k, "queries": n,
           "calls": a.calls, "forms": {}}
    got = {}
    ok = True
    for form, roles in (("must_must", ("must", "must")), ("must_should", ("must", "should")),
                        ("should_should", ("should", "should"))):
        arr = (_capi.BoolQuery * n)(*[eng.resolve_bool(w.BoolQuery(list(zip(t, roles)), n_results=a.k))[0]
                                      for t in items])
        counts, cst = (C.c_int64 * n)(), _capi.OrStats()
        hits, nh, bst = (_capi.Hit * (n * a.k))(), (C.c_int32 * n)(), _capi.OrStats()

        def count_step():
            _capi.check(lib.wsr_count_bool_ex(eng._h, arr, n, counts, 0, C.byref(cst)))

        def bool_step():
            _capi.check(lib.wsr_search_bool_ex(eng._h, arr, n, a.k, hits, nh, 0, C.byref(bst)))

        cts = timed(count_step)
        bts = timed(bool_step)
        cms = statistics.median(cts)
        got[form] = list(counts)
        bad = sum(1 for c, h in zip(counts, nh) if c < h or (c <= a.k and c != h))
        holds = cms <= min(bts)
        ok = ok and holds and not bad
        out["forms"][form] = {
            "count": {"value": round(n / (cms * 1e-3), 1), "unit": "queries/s", "median_ms": round(cms, 3),
                      "calls_ms": [round(x, 3) for x in cts], "stats": stats_of(cst),
                      "matches": sum(counts), "max": max(counts)},
            "search_bool": {"median_ms": round(statistics.median(bts), 3), "fastest_ms": round(min(bts), 3),
                            "calls_ms": [round(x, 3) for x in bts], "stats": stats_of(bst)},
            "count_median_at_most_fastest_search_bool": holds,
            "mismatches_vs_n_hits": bad}
        print(f"[count_bench] {form}: count {cms:.3f} ms, wsr_search_bool fastest {min(bts):.3f} ms",
              file=sys.stderr, flush=True)

    df = [[eng.lookup(x)[1] for x in t] for t in items]
    out["mismatches_or_identity"] = sum(1 for d, n_and, n_or in zip(df, got["must_must"], got["should_should"])
                                        if n_or != d[0] + d[1] - n_and)
    out["mismatches_must_should"] = sum(1 for d, c in zip(df, got["must_should"]) if c != d[0])
    ok = ok and not out["mismatches_or_identity"] and not out["mismatches_must_should"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    eng.close()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
