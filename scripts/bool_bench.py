#!/usr/bin/env python3
"""Throughput of boolean queries (wsr_search_bool) on the C3 stand-in.

Runs the first --queries queries of the two-term log that `bench.py --prepare`
writes under $WISER_BENCH_DIR (or bench.py's default index directory), k = 10,
as one wsr_search_bool call per step, in three forms: both terms MUST, the
first MUST and the second SHOULD, both SHOULD.  Per form: a warm-up call, then
the median of --calls timed calls (a call is synchronous: copies in, kernel,
replay, copies out, one wait).  For the both-SHOULD form the same queries also
run as WSR_QUERY_OR in one resident batch (run + fetch per step), the figure
the boolean call must stay near: a call adds the copies of its tables and
results to the same traversal.  The all-MUST answers are compared with the
conjunctive SearchBatch, the all-SHOULD ones with the OR batch, bit for bit.
Writes one JSON object (--out, default profiles/bool/bench.json) and prints it.
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bool", "bench.json"))
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

    def median_ms(step):
        step()   # warm-up: the context's buffers grow here
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            step()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts

    out = {"workload": "c3_two_term_bool", "index": os.path.basename(idx), "k": a.k, "queries": n,
           "calls": a.calls, "forms": {}}
    answers = {}
    for form, roles in (("must_must", ("must", "must")), ("must_should", ("must", "should")),
                        ("should_should", ("should", "should"))):
        arr = (_capi.BoolQuery * n)(*[eng.resolve_bool(w.BoolQuery(list(zip(t, roles)), n_results=a.k))[0]
                                      for t in items])
        hits, nh, st = (_capi.Hit * (n * a.k))(), (C.c_int32 * n)(), _capi.OrStats()

        def step():
            _capi.check(lib.wsr_search_bool_ex(eng._h, arr, n, a.k, hits, nh, 0, C.byref(st)))

        ms, ts = median_ms(step)
        answers[form] = [[(hits[i * a.k + j].score, hits[i * a.k + j].doc_id) for j in range(nh[i])]
                         for i in range(n)]
        out["forms"][form] = {"value": round(n / (ms * 1e-3), 1), "unit": "queries/s", "median_ms": round(ms, 3),
                              "calls_ms": [round(x, 3) for x in ts],
                              "stats": {"items": st.items, "windows": st.windows,
                                        "windows_skipped": st.windows_skipped, "touched_docs": st.touched_docs,
                                        "events": st.events}}
        print(f"[bool_bench] {form}: {out['forms'][form]['value']} q/s", file=sys.stderr, flush=True)

    # the same queries as WSR_QUERY_OR in one resident batch: run + fetch per step
    b = w.ResidentBatch(eng, n, a.k)
    b.upload((_capi.Query * n)(*[eng.resolve(w.SearchQuery(t, n_results=a.k, match_any=True))[0] for t in items]))
    res = {}

    def or_step():
        b.run()
        res["hits"], res["nh"] = b.fetch()

    ms, ts = median_ms(or_step)
    out["or_resident_batch"] = {"value": round(n / (ms * 1e-3), 1), "unit": "queries/s", "median_ms": round(ms, 3),
                                "calls_ms": [round(x, 3) for x in ts]}
    # (fetch returns views of the batch's page-locked arrays: read them before the batch closes)
    or_ans = [[(res["hits"][i * a.k + j].score, res["hits"][i * a.k + j].doc_id) for j in range(res["nh"][i])]
              for i in range(n)]
    b.close()
    and_res = eng.SearchBatch([w.SearchQuery(t, n_results=a.k) for t in items])
    and_ans = [[(e.doc_score, e.doc_id) for e in r.entries] for r in and_res]
    out["mismatches_should_vs_or"] = sum(1 for x, y in zip(answers["should_should"], or_ans) if x != y)
    out["mismatches_must_vs_and"] = sum(1 for x, y in zip(answers["must_must"], and_ans) if x != y)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    eng.close()
    if out["mismatches_should_vs_or"] or out["mismatches_must_vs_and"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
