#!/usr/bin/env python3
"""Throughput of wsr_score_docs on bench.py's C3 stand-in index: the first
4,096 queries of the two-term log, per query its conjunctive top-64 plus 960
pseudo-random doc ids (a re-ranker's candidate set: the hits and a crowd of
misses), all in one call.

Reports pairs/s and ms per call (the median of --reps calls after a warm-up
call; a call is synchronous: plan on the host, copies, kernel, copy back), and
the share of a call's time spent in score_docs_kernel, taken from one
`rocprofv3 --kernel-trace --stats` run of this script's own (--child: the same
calls, nothing timed).  One MI355X, one run form.  Writes one JSON file
(default profiles/score_docs/bench.json) and prints it.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP, RANDOM = 64, 960


def workload(n_queries):
    """-> (engine, queries, doc_off, docs, out) as ctypes arrays"""
    import numpy as np
    import bench
    import wiser_amd as w
    from wiser_amd import _capi
    a = argparse.Namespace(index_dir=bench.default_index_dir(), c3_docs=5_500_000, c3_term_scale=1.0)
    d, qlog, _ = bench.ensure_c3(a)
    eng = w.VacuumEngine(d, positions=False)
    eng.Load()
    lines = [t for t, _ in w.read_query_log(qlog)[:n_queries]]
    res = eng.SearchBatch([w.SearchQuery(t, n_results=TOP) for t in lines])
    rng = np.random.default_rng(7)
    n_docs = eng.NumDocs()
    lists = [np.concatenate([np.array([e.doc_id for e in r.entries], dtype=np.int32),
                             rng.integers(0, n_docs, RANDOM, dtype=np.int32)]) for r in res]
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    docs = np.ascontiguousarray(np.concatenate(lists))
    arr = (_capi.Query * len(lines))(*[eng.resolve_terms(w.SearchQuery(t)) for t in lines])
    out = (_capi.DocScore * len(docs))()
    return eng, arr, off, docs, out


def call(eng, arr, off, docs, out):
    from wiser_amd import _capi
    _capi.check(_capi.lib.wsr_score_docs(eng._h, arr, len(arr), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                         docs.ctypes.data_as(C.POINTER(C.c_int32)), out))


def kernel_ns_per_call(args):
    """score_docs_kernel's average duration in a rocprofv3 run of --child"""
    tmp = tempfile.mkdtemp(prefix="wsr_score_prof")
    try:
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o",
                               "score", "--", sys.executable, os.path.abspath(__file__), "--child", "--queries",
                               str(args.queries), "--reps", str(args.reps)], stdout=subprocess.DEVNULL)
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "score_docs_kernel" in row["Name"]:
                    return float(row["TotalDurationNs"]) / float(row["Calls"]), int(row["Calls"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    raise SystemExit("no score_docs_kernel row in the kernel stats")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=4096)
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_docs", "bench.json"))
    p.add_argument("--child", action="store_true", help="the calls alone (the run rocprofv3 traces)")
    args = p.parse_args()
    eng, arr, off, docs, out = workload(args.queries)
    call(eng, arr, off, docs, out)   # warm-up: the context's buffers are allocated
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        call(eng, arr, off, docs, out)
        times.append(time.perf_counter() - t)
    import numpy as np
    masks = np.frombuffer(out, dtype=[("score", "<f8"), ("mask", "<u4"), ("pad", "<i4")])["mask"]
    full, some = int((masks == 3).sum()), int((masks != 0).sum())
    eng.close()
    if args.child:
        return
    ms = statistics.median(times) * 1e3
    k_ns, k_calls = kernel_ns_per_call(args)
    result = {
        "what": "wsr_score_docs, one MI355X, one run form: one synchronous call per repetition",
        "index": "bench.py C3 stand-in (5,500,000 docs), first queries of its two-term log",
        "queries": len(arr), "pairs": int(len(docs)),
        "candidates_per_query": f"conjunctive top-{TOP} + {RANDOM} pseudo-random doc ids",
        "pairs_full_mask": full, "pairs_any_mask": some,
        "reps": args.reps, "ms_per_call_median": round(ms, 3),
        "ms_per_call_min": round(min(times) * 1e3, 3), "ms_per_call_max": round(max(times) * 1e3, 3),
        "pairs_per_s": round(len(docs) / (ms * 1e-3)),
        "kernel_ms_per_call": round(k_ns * 1e-6, 3), "kernel_calls_traced": k_calls,
        "kernel_share_of_call": round(k_ns * 1e-6 / ms, 4),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
