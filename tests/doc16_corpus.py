"""The hand-made corpus of the 16-bit doc id tests (test_doc16_image.py,
test_gpu_doc16.py; next to edge_corpora.py).  680,000 docs of a few tokens
each, TOKEN_ONLY.  The size is what a bucket O1 needs: offset buckets are
built below 2.5 % density, and an O1 is no shorter than its driver, so a driver
of 127 blocks (16,256 postings) needs an O1 of as many postings in more than
650,240 docs.

  z     every doc but those with id % 7 == 3: a bitmap O1, and a third term
  ob    every 41st doc (16,586 postings, 130 blocks, 2.44 %): a bucket O1
  d127, d64, d63   drivers of exactly 127, 64 and 63 pack blocks, no tail,
        about half of their postings in docs of ob
  d2t   2 pack blocks and a VInts tail of 50
  s     block 1 spans exactly 65,535 docs (its last posting's offset is
        0xFFFF, in a doc of z); then a tail of 10
  t     as s with that posting one doc later: the span is 65,536
  f     200 postings from doc 40,001 on (its first block starts far from 0)
  g     130 postings from doc 66,000 on
  p     one pack block, then a VInts tail of 5
  q     50 postings: a VInts block alone
A driver's tf is 1 + j % 3 for its j-th posting (12 for the last posting of
block 1 of s and t); docs have 0..4 filler words.
"""
import os

N_DOCS = 680_000
EDGE_TF = 12
OB_STRIDE = 41
SPAN = 65_535


def _driver(n, stride, base, alt, period):
    """n postings: base + stride * j, every period-th moved alt docs on"""
    return [base + stride * j + (alt if j % period == period - 1 else 0) for j in range(n)]


def _edge(last_of_block1):
    b0 = [OB_STRIDE * j for j in range(128)]
    b1 = [b0[-1] + OB_STRIDE * (j + 1) for j in range(127)] + [last_of_block1]
    return b0 + b1 + [last_of_block1 + OB_STRIDE * (j + 1) for j in range(10)]


def lists():
    """term -> ascending doc ids of the hand-made lists (z and ob are by rule)"""
    e0 = OB_STRIDE * 127
    out = {
        "d127": _driver(127 * 128, 41, 0, 1, 2),
        "d64": _driver(64 * 128, 82, 0, 1, 3),
        "d63": _driver(63 * 128, 82, 41, 2, 3),
        "d2t": _driver(2 * 128 + 50, 41, 1025, 1, 4),
        "s": _edge(e0 + SPAN),
        "t": _edge(e0 + SPAN + 1),
        "f": [40_001 + 3 * j for j in range(200)],
        "g": [66_000 + 5 * j for j in range(130)],
        "p": [7 + 3 * j for j in range(128 + 5)],
        "q": [11 + 9 * j for j in range(50)],
    }
    for t, docs in out.items():
        assert docs == sorted(set(docs)) and docs[-1] < N_DOCS, t
    return out


def build_index(root):
    """-> index dir"""
    import wiser_amd as w
    root = str(root)
    per_doc = {}
    for t, docs in lists().items():
        for j, d in enumerate(docs):
            # (the posting at the span's edge scores high, so that it is among a query's results)
            per_doc.setdefault(d, []).extend([t] * (EDGE_TF if t in "st" and j == 255 else 1 + j % 3))
    ld = os.path.join(root, "doc16.linedoc")
    with open(ld, "w") as f:
        f.write("FIELDS_HEADER_INDICATOR###\tdoctitle\tbody\ttokenized\n")
        for i in range(N_DOCS):
            toks = per_doc.get(i, [])
            if i % 7 != 3:
                toks = toks + ["z"]
            if i % OB_STRIDE == 0:
                toks = toks + ["ob"]
            toks = toks + [f"f{x}" for x in range(i % 5)] if toks or i % 5 else ["f0"]
            body = " ".join(toks)
            f.write(f"t\t{body}\t{body}\n")
    d = os.path.join(root, "idx")
    os.makedirs(d)
    w.build_from_linedoc(ld, d, "TOKEN_ONLY")
    return d


def doc16(index_dir, term, doc_range=(0, 0), max_blocks=256):
    """-> (eligible, blocks of the list in the image, [prev of each block], [its 128 slots] or
    None when not eligible), for the first max_blocks blocks (wsr_debug_doc16)"""
    return doc16_probe(index_dir, term, doc_range, max_blocks)[:4]


def doc16_probe(index_dir, term, doc_range=(0, 0), max_blocks=1):
    """doc16()'s tuple and the list's probe structure in the image: -1 none, 0 a
    rank bitmap, else the shift of its offset buckets"""
    import ctypes as C
    from wiser_amd._capi import check, lib
    out = (C.c_uint16 * (128 * max_blocks))()
    prev = (C.c_uint32 * max_blocks)()
    nb, ok, probe = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.wsr_debug_doc16(index_dir.encode(), doc_range[0], doc_range[1], term.encode(), max_blocks, out,
                              prev, C.byref(nb), C.byref(ok), C.byref(probe)))
    n = min(nb.value, max_blocks)
    slots = [list(out[128 * b:128 * b + 128]) for b in range(n)] if ok.value else None
    return bool(ok.value), nb.value, list(prev[:n]), slots, probe.value
