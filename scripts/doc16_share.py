"""Share of a leg's driver blocks that 16-bit doc ids could serve (DESIGN.md
10.2): a block is eligible when it is a full pack block whose last - prev is at
most 65,535, a list when every pack block of it is (its VInts tail block is not
counted).  Every query of the leg's log is given its driver by the plan's rule
(the list of the fewest blocks, the first of equals) and weighed by the
driver's blocks in the whole index; per batch, the share of those blocks that
belong to eligible lists, and the share that are eligible blocks themselves,
which is what a per-block rule could reach at most.  Host only: the skip rows
of the index, no image, no GPU.  Prints one JSON line.

Legs: those of scripts/leg_run.py (its open_leg picks the index and the log).

usage: doc16_share.py LEG"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def survey(idx, terms):
    """-> {term: (blocks, eligible pack blocks, the list is eligible by the loader's rule)} (wsr_doc16_survey)"""
    from wiser_amd._capi import check, lib
    terms = sorted(terms)
    n = len(terms)
    arr = (C.c_char_p * n)(*[t.encode() for t in terms])
    nb, npk, ok = ((C.c_uint32 * n)() for _ in range(3))
    el = (C.c_int32 * n)()
    check(lib.wsr_doc16_survey(idx.encode(), arr, n, nb, npk, ok, el))
    return {t: (nb[i], ok[i], bool(el[i])) for i, t in enumerate(terms)}


def main():
    import bench
    from leg_run import ALIASES, open_leg
    leg = ALIASES.get(sys.argv[1], sys.argv[1])
    sys.argv = [sys.argv[0], "--no-cpu"]
    a = bench.parse()
    idx, items, _, _ = open_leg(a, leg)
    info = survey(idx, {t for terms, _ in items for t in terms})
    rows = []   # per batch: driver blocks, those of eligible lists, eligible blocks
    for s in range(0, len(items), a.batch):
        db = dl = dk = 0
        for terms, phrase in items[s:s + a.batch]:
            lists = [info[t] for t in terms]
            if phrase or len(lists) < 2 or any(l[0] == 0 for l in lists):
                continue   # (not a conjunctive item with a probe; a missing term: an empty query)
            nb, ok, eligible = min(lists, key=lambda l: l[0])   # (min keeps the first of equals)
            db += nb
            dl += nb if eligible else 0
            dk += ok
        rows.append((db, dl, dk))
    db, dl, dk = (sum(r[i] for r in rows) for i in range(3))
    per_list = sorted(r[1] / max(r[0], 1) for r in rows)
    per_block = sorted(r[2] / max(r[0], 1) for r in rows)
    print(json.dumps({"leg": leg, "batches": len(rows), "batch": a.batch,
                      "driver_blocks_per_batch": round(db / max(len(rows), 1), 1),
                      "list_share": round(dl / max(db, 1), 4),
                      "list_share_min": round(per_list[0], 4) if rows else None,
                      "list_share_max": round(per_list[-1], 4) if rows else None,
                      "block_share": round(dk / max(db, 1), 4),
                      "block_share_min": round(per_block[0], 4) if rows else None,
                      "block_share_max": round(per_block[-1], 4) if rows else None,
                      "list_share_per_batch": [round(r[1] / max(r[0], 1), 4) for r in rows],
                      "block_share_per_batch": [round(r[2] / max(r[0], 1), 4) for r in rows],
                      "src_sha": bench.src_sha()}))


if __name__ == "__main__":
    main()
