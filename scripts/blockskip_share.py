"""Share of a leg's driver blocks that skipping whole blocks on a per-block
impact maximum could leave out at most: every batch of the
leg's log runs once, alone, and its statistics give the driver blocks its items
ran (wsr_batch_stats::driver_blocks, the general kernel's included where a
batch launches it) and, of them, the conjunctive lean pipeline's blocks whose D
stage kept no posting (skippable_blocks).  Prints one JSON line.

Legs: those of scripts/leg_run.py (its open_leg picks the index and the log).

usage: blockskip_share.py LEG"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import bench
    from leg_run import ALIASES, open_leg
    leg = ALIASES.get(sys.argv[1], sys.argv[1])
    sys.argv = [sys.argv[0], "--no-cpu"]
    a = bench.parse()
    import wiser_amd as w
    from wiser_amd import _capi
    idx, items, _, positions = open_leg(a, leg)
    eng = w.VacuumEngine(idx, device=0, threads=bench.HOST_THREADS, positions=positions)
    eng.Load()
    rows = []
    for s in range(0, len(items), a.batch):
        chunk = items[s:s + a.batch]
        arr = (_capi.Query * len(chunk))()
        for i, (terms, ph) in enumerate(chunk):
            arr[i] = eng.resolve(w.SearchQuery(terms, n_results=a.k, is_phrase=ph))[0]
        b = w.ResidentBatch(eng, a.batch, a.k)
        b.upload(arr)
        b.run()
        b.fetch()
        st = b.stats()
        b.close()
        rows.append((st.driver_blocks, st.skippable_blocks, st.survivors))
    eng.close()
    db, sk, sv = (sum(r[i] for r in rows) for i in range(3))
    shares = sorted(r[1] / max(r[0], 1) for r in rows)
    print(json.dumps({"leg": leg, "batches": len(rows), "batch": a.batch, "k": a.k,
                      "driver_blocks_per_batch": round(db / max(len(rows), 1), 1),
                      "skippable_blocks_per_batch": round(sk / max(len(rows), 1), 1),
                      "survivors_per_batch": round(sv / max(len(rows), 1), 1),
                      "skippable_share": round(sk / max(db, 1), 4),
                      "skippable_share_min": round(shares[0], 4) if shares else None,
                      "skippable_share_max": round(shares[-1], 4) if shares else None,
                      "src_sha": bench.src_sha()}))


if __name__ == "__main__":
    main()
