"""Share of a leg's queries that the tiny class takes (DESIGN.md 4q and
5.0000000): per batch of the leg's log, the queries that meet is_tiny_query
(engine_types.h: two terms, both lists one VInts block, i.e. 1 <= df <= 127 in
the whole index), the general queries that are left (a conjunctive query whose
other lists do not all carry a bitmap or buckets; a list carries one when
df * dense_div >= docs, the loader's rule without its HBM budget), and the
share of those left whose two lists' doc-id ranges do not meet.  Host only:
document frequencies and postings from the oracle's reader, no image, no GPU.
Prints one JSON line.

Legs: those of scripts/leg_run.py (its open_leg picks the index and the log).

usage: tiny_share.py LEG [DENSE_DIV]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import bench
    from leg_run import ALIASES, open_leg
    from oracle.oracle import OracleVacuum
    leg = ALIASES.get(sys.argv[1], sys.argv[1])
    dense_div = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    sys.argv = [sys.argv[0], "--no-cpu"]
    a = bench.parse()
    idx, items, _, _ = open_leg(a, leg)
    orc = OracleVacuum(idx)
    n_docs = orc.n_docs()
    df = {t: orc.df(t) for terms, _ in items for t in terms}
    blocks = {t: (n + 127) // 128 for t, n in df.items()}
    has_bm = {t: n * dense_div >= n_docs for t, n in df.items()}
    span = {}

    def doc_span(t):
        if t not in span:
            docs = orc.postings(t)[0]
            span[t] = (docs[0], docs[-1])
        return span[t]

    rows = []   # per batch: queries, tiny, general left, of those disjoint
    for s in range(0, len(items), a.batch):
        n_tiny = n_gen = n_disjoint = 0
        batch = items[s:s + a.batch]
        for terms, phrase in batch:
            if not terms or any(df[t] == 0 for t in terms):
                continue   # an empty query
            if len(terms) == 2 and not phrase and all(1 <= df[t] <= 127 for t in terms):
                n_tiny += 1
                continue
            drv = min(range(len(terms)), key=lambda i: blocks[terms[i]])   # (the first of equals)
            lean = all(has_bm[t] for i, t in enumerate(terms) if i != drv) and not (phrase and len(terms) > 2)
            if lean:
                continue
            n_gen += 1
            if len(terms) == 2:
                (a0, a1), (b0, b1) = doc_span(terms[0]), doc_span(terms[1])
                n_disjoint += a0 > b1 or b0 > a1
        rows.append((len(batch), n_tiny, n_gen, n_disjoint))
    orc.close()
    nq, nt, ng, nd = (sum(r[i] for r in rows) for i in range(4))
    print(json.dumps({"leg": leg, "batches": len(rows), "batch": a.batch, "dense_div": dense_div, "docs": n_docs,
                      "queries": nq, "tiny": nt, "tiny_share": round(nt / max(nq, 1), 4),
                      "general_left": ng, "general_left_share": round(ng / max(nq, 1), 4),
                      "general_left_disjoint_share": round(nd / max(ng, 1), 4),
                      "tiny_per_batch": [r[1] for r in rows],
                      "general_left_per_batch": [r[2] for r in rows],
                      "general_left_disjoint_share_per_batch": [round(r[3] / max(r[2], 1), 4) for r in rows],
                      "src_sha": bench.src_sha()}))


if __name__ == "__main__":
    main()
