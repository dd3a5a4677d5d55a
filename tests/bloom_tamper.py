"""Tampering with the two-way phrase bloom filters of a written index (next to
edge_corpora.py): honest filters have no false negatives, so a bloom-pruned
phrase path that reads the wrong posting's filter, the wrong side or none
changes a result only where some filters are missing.  blank_bloom_boxes takes
them away box by box."""
import os
import struct


def _varint(b, i):
    v = sh = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << sh
        sh += 7
        if not c & 0x80:
            return v, i


def _list_offsets(index_dir):
    """{term: offset of its posting list in my.vacuum} from my.tip"""
    tip = open(os.path.join(index_dir, "my.tip"), "rb").read()
    offs, at = {}, 0
    while at < len(tip):
        n = struct.unpack_from("<I", tip, at)[0]
        t = tip[at + 4:at + 4 + n].decode()
        v = struct.unpack_from("<q", tip, at + 4 + n)[0]
        offs[t] = v & ((1 << 48) - 1)
        at += 4 + n + 8
    return offs


def bloom_box_count(index_dir, term):
    """Boxes of the term's bloom sections (one per 128 postings)."""
    o = _list_offsets(index_dir)[term]
    vac = open(os.path.join(index_dir, "my.vacuum"), "rb").read()
    assert vac[o] == 0xF4
    _, i = _varint(vac, o + 1)
    s0, _ = _varint(vac, i)
    assert vac[o + s0] == 0xA4
    return _varint(vac, o + s0 + 1)[0]


def blank_bloom_boxes(index_dir, boxes):
    """boxes = {term: box indices} (a negative index counts from the term's
    last box; box b holds the filters of postings [128 b, 128 b + 128)).  Mark
    every posting of those boxes, in both sections (prior and next), as having
    no filter: the box's presence bitmap zeroed in place (the arrays stay but
    nothing points at them).  The reference's reader then answers "not present"
    for those postings (flash_iterators.h:1045-1050).
    -> {term: the sorted box indices blanked, all >= 0}"""
    offs = _list_offsets(index_dir)
    path = os.path.join(index_dir, "my.vacuum")
    vac = bytearray(open(path, "rb").read())
    done = {}
    for t, idxs in boxes.items():
        o = offs[t]
        assert vac[o] == 0xF4
        _, i = _varint(vac, o + 1)
        s0, i = _varint(vac, i)
        s1, _ = _varint(vac, i)
        for s in (s0, s1):
            p = o + s
            assert vac[p] == 0xA4
            nbox, p = _varint(vac, p + 1)
            want = sorted({b + nbox if b < 0 else b for b in idxs})
            assert want and 0 <= want[0] and want[-1] < nbox, (t, idxs, nbox)
            assert done.setdefault(t, want) == want   # (both sections have a box per skip row)
            at = 0
            for b in range(want[-1] + 1):
                d, p = _varint(vac, p)
                at += d
                if b not in want:
                    continue
                bx = o + at
                assert vac[bx] == 0xF5
                n, q = _varint(vac, bx + 1)
                vac[q:q + (n + 7) // 8] = bytes((n + 7) // 8)
    open(path, "wb").write(bytes(vac))
    return done


# ---- the tampered copies of the edge corpora (edge_corpora.py) ---------------
def tie_blanks(index_dir):
    """The tie corpus: of each of a, b, c and d the boxes 0 and 1, every box b
    with b % 7 == 3 and the last one.  "a" is in every doc, so its posting index
    is the doc id, box 0 is docs [0, 128) and box 1 opens at doc 128; the
    posting index of b, c and d runs behind the doc id, so a filter read by doc
    id or by the row of the whole list lands in a box of the other kind."""
    out = {}
    for t in "abcd":
        n = bloom_box_count(index_dir, t)
        out[t] = sorted({0, 1, n - 1} | {b for b in range(n) if b % 7 == 3})
    return out


# the skewed corpus of seed 1: first boxes (x128: its only box, full) and last
# boxes (x129: a box of one posting; x300: of 44)
RAND1_BLANKS = {"v0": [0], "heavy": [0], "x128": [0], "v1": [-1], "x129": [-1], "x300": [-1]}


def tampered_copy(src, dst, corpus):
    """The bloom index src of corpus "tiespos" / "rand1" copied to dst with the
    boxes above blanked -> {term: box indices blanked}"""
    import shutil
    shutil.copytree(src, dst)
    return blank_bloom_boxes(dst, tie_blanks(dst) if corpus == "tiespos" else RAND1_BLANKS)
