#!/usr/bin/env python3
"""Throughput of disjunctive (OR) queries on the C3 stand-in.

Runs the two-term log that `bench.py --prepare` writes under $WISER_BENCH_DIR
(or bench.py's default index directory) as WSR_QUERY_OR queries: k = 10,
resident batches, 5 warm-up and 20 timed steps (a step = one run of one batch,
consecutive batches in flight).  The batch is the largest prefix-sized batch
(a power of two, at most --max-batch) whose worst-case event slots -- every
posting of both lists an event -- fit --event-gib for all resident batches.
Prints one JSON line: q/s, ms per step, the OR statistics of one batch and its
algorithmic bytes per step over the step time as a fraction of 8 TB/s.  After
the timed loop, --check queries of the last run are compared, bit for bit, with
the oracle's per-term contributions summed in query order and ranked by the
restated heap (tests/heapmodel.py).

There is no reference figure for OR: the number stands beside the same log's
AND figure (bench.py --full) only to show the cost of answering a different
question (every doc of both lists is scored, not their intersection).
"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GBS = 8000.0


def rank_fast(scores, docs, k):
    """heapmodel.rank_stream over (score, doc) arrays in doc order: the heap's
    minimum only grows, so of each chunk only the items above the minimum at
    the chunk's start can be insertions; those go through the heap one by one."""
    from heapmodel import Heap
    h = Heap()
    n = len(docs)
    i = 0
    while i < n and len(h.v) < k:
        h.push((float(scores[i]), int(docs[i])))
        i += 1
    while i < n:
        j = min(n, i + 65536)
        top = h.v[0][0]
        sel = (scores[i:j] > top).nonzero()[0]
        for x in sel:
            s = float(scores[i + x])
            if s > h.v[0][0]:
                h.pop()
                h.push((s, int(docs[i + x])))
        i = j
    out = []
    while h.v:
        out.append(h.v[0])
        h.pop()
    return out[::-1]


def expected(orc, cache, terms, k):
    import numpy as np
    parts = []
    for t in terms:
        if t not in cache:
            df = orc.df(t)
            if df > 0:
                res = orc.search([t], df)[0]
                d = np.fromiter((x[0] for x in res), dtype=np.int64, count=len(res))
                s = np.fromiter((x[1] for x in res), dtype=np.float64, count=len(res))
                o = np.argsort(d, kind="stable")
                cache[t] = (d[o], s[o])
            else:
                cache[t] = None
        if cache[t] is not None:
            parts.append(cache[t])
    if not parts:
        return []
    docs = np.unique(np.concatenate([p[0] for p in parts]))
    acc = np.zeros(len(docs), dtype=np.float64)
    for d, s in parts:   # query order; a repeated term is added again
        acc[np.searchsorted(docs, d)] += s
    return rank_fast(acc, docs, k)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--index-dir", default=None, help="the C3 stand-in (default: found under bench.py's index dir)")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--resident", type=int, default=4, help="resident batches (distinct slices of the log)")
    p.add_argument("--max-batch", type=int, default=4096)
    p.add_argument("--event-gib", type=float, default=48.0, help="event slots of all resident batches at most")
    p.add_argument("--check", type=int, default=256)
    a = p.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process, as bench.py)
    import bench
    import wiser_amd as w
    from wiser_amd import _capi
    idx = a.index_dir
    if not idx:
        found = sorted(glob.glob(os.path.join(bench.default_index_dir(), "c3_wiki_*", "READY")))
        if not found:
            raise SystemExit("no C3 stand-in: run `python bench.py --prepare` first")
        idx = os.path.dirname(found[0])
    log = os.path.join(idx, "two_term_100000.log")
    items = [t for t, ph in w.read_query_log(log) if not ph]
    eng = w.VacuumEngine(idx, positions=False)
    eng.Load()

    def resolve(terms):
        return eng.resolve(w.SearchQuery(terms, n_results=a.k, match_any=True))

    # worst-case events of a query: every posting of its lists (+ a block per item and list)
    need, qs = [], []
    for terms in items[:a.max_batch * a.resident]:
        q, dfs = resolve(terms)
        qs.append(q)
        need.append(sum(dfs or []) + 256)
    budget = a.event_gib * 2 ** 30 / 16 / 1.3   # (the upload allocates a quarter more)
    batch = a.max_batch
    while batch > 1 and sum(need[:batch * a.resident]) > budget:
        batch //= 2
    batches = []
    for r in range(a.resident):
        arr = (_capi.Query * batch)(*qs[r * batch:(r + 1) * batch])
        b = w.ResidentBatch(eng, batch, a.k)
        b.upload(arr)
        batches.append(b)
    for s in range(a.warmup):
        batches[s % a.resident].run()
    w.sync(eng)
    t0 = time.perf_counter()
    for s in range(a.steps):
        batches[s % a.resident].run()
    w.sync(eng)
    el = time.perf_counter() - t0
    st, ost = batches[0].stats(), batches[0].or_stats()
    last = (a.steps - 1) % a.resident
    hits, nh = batches[last].fetch()   # (raises on a device error flag, e.g. a full event slot)
    for i, b in enumerate(batches):
        if i != last:
            b.fetch()
    ms = el / a.steps * 1e3
    out = {"workload": "c3_two_term_or", "index": os.path.basename(idx), "k": a.k, "batch": batch,
           "batches_resident": a.resident, "warmup": a.warmup, "steps": a.steps,
           "event_slots_gib": round(sum(need[:batch * a.resident]) * 16 * 1.25 / 2 ** 30, 2),
           "value": round(batch * a.steps / el, 1), "unit": "queries/s", "ms_per_step": round(ms, 3),
           "or_stats_per_batch": {"items": ost.items, "windows": ost.windows,
                                  "windows_skipped": ost.windows_skipped, "touched_docs": ost.touched_docs,
                                  "events": ost.events},
           "algo_bytes_per_batch": st.algo_bytes,
           "achieved_gbs": round(st.algo_bytes / (ms * 1e-3) / 1e9, 1),
           "frac_of_8tbs": round(st.algo_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    # parity of the last timed run against the model, after the timed loop
    from oracle.oracle import OracleVacuum
    orc = OracleVacuum(idx)
    cache, bad, n = {}, 0, min(a.check, batch)
    for i in range(n):
        terms = items[last * batch + i]
        got = [(hits[i * a.k + j].score, hits[i * a.k + j].doc_id) for j in range(nh[i])]
        if got != expected(orc, cache, terms, a.k):
            bad += 1
            print(f"[or_bench] MISMATCH {terms}", file=sys.stderr, flush=True)
        if i % 16 == 15:
            print(f"[or_bench] checked {i + 1}/{n}", file=sys.stderr, flush=True)
        if len(cache) > 64:
            cache.clear()
    out["parity_checked_queries"] = n
    out["parity_mismatches"] = bad
    print(json.dumps(out), flush=True)
    for b in batches:
        b.close()
    eng.close()
    orc.close()
    if bad:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
