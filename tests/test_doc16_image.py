"""The 16-bit doc ids of the image (HostImage::doc16, engine_types.h): slot p
of block b holds doc(b, p) - BlockDev::prev(b) for the lists whose pack blocks
each span at most 65,535 docs.  Host only (wsr_debug_doc16 builds the image
wsr_open would, without a device), on the hand-made corpus of doc16_corpus.py;
the doc ids are the oracle's, decoded from the file.
"""
import os

import pytest

import doc16_corpus as dc


@pytest.fixture(scope="module")
def corpus(built, tmp_path_factory):
    from oracle.oracle import OracleVacuum
    d = dc.build_index(tmp_path_factory.mktemp("doc16"))
    orc = OracleVacuum(d)
    docs = {t: orc.postings(t)[0] for t in list(dc.lists()) + ["ob"]}
    orc.close()
    return d, docs


def test_lists_are_what_the_cases_need(corpus):
    _, docs = corpus
    want = dc.lists()
    for t in want:
        assert docs[t] == want[t], t
    s, t = docs["s"], docs["t"]
    assert s[255] - s[127] == 65_535 and t[255] - t[127] == 65_536 and s[:255] == t[:255]
    assert len(docs["p"]) == 128 + 5 and len(docs["q"]) == 50 and len(docs["d2t"]) == 2 * 128 + 50


@pytest.mark.parametrize("term", sorted(dc.lists()) + ["ob"])
def test_offsets_give_the_doc_ids(corpus, term):
    """Eligible exactly when every pack block (128 postings; a shorter last
    block is the VInts tail) spans at most 65,535 docs from the prev the image
    holds for it, and there is one; then prev + slot is the doc id of every
    posting of every pack block, the first block included."""
    d, docs = corpus
    ids = docs[term]
    npk, nblk = len(ids) // 128, (len(ids) + 127) // 128
    ok, n, prevs, slots = dc.doc16(d, term)
    assert n == nblk == len(prevs)
    assert all(prevs[b] == ids[128 * b - 1] for b in range(1, nblk))
    assert prevs[0] <= ids[0]
    want = npk > 0 and all(ids[128 * b + 127] - prevs[b] <= 65_535 for b in range(npk))
    assert ok == want, (term, want)
    if ok:
        for b in range(npk):
            assert [prevs[b] + o for o in slots[b]] == ids[128 * b:128 * b + 128], (term, b)
        if nblk > npk:   # the VInts tail block's slots are never read as ids: zeros
            assert slots[npk] == [0] * 128


def test_span_edge(corpus):
    d, _ = corpus
    ok, _, prevs, slots = dc.doc16(d, "s")
    assert ok and slots[1][127] == 0xFFFF and prevs[1] + 0xFFFF == dc.lists()["s"][255]
    assert not dc.doc16(d, "t")[0]


def test_expected_eligibility(corpus):
    d, _ = corpus
    for t in ("d127", "d64", "d63", "d2t", "s", "f", "p", "ob"):
        assert dc.doc16(d, t)[0], t
    for t in ("t", "q"):   # a span of 65,536; no pack block
        ok, _, _, slots = dc.doc16(d, t)
        assert not ok and slots is None, t
    # one pack block followed by a VInts tail: eligible on the pack block alone
    ok, nblk, _, _ = dc.doc16(d, "p")
    assert ok and nblk == 2


def test_shard_image_offsets_are_from_the_blocks_own_prev(corpus):
    """A doc-range image holds the blocks that can meet its range, numbered
    from its first; their slots are the same offsets."""
    d, docs = corpus
    ids = docs["d127"]
    lo, hi = 340_000, dc.N_DOCS
    first = next(b for b in range(127) if ids[128 * b + 127] >= lo)
    assert ids[128 * first] < lo   # the cut falls inside the block
    ok, nblk, prevs, slots = dc.doc16(d, "d127", (lo, hi))
    assert ok and nblk == 127 - first and prevs[0] == ids[128 * first - 1]
    for b in (0, 1, nblk - 1):
        assert [prevs[b] + o for o in slots[b]] == ids[128 * (first + b):128 * (first + b) + 128]


def test_doc16_off_builds_nothing(corpus):
    import wiser_amd as w
    d, _ = corpus
    on = w.image_size(d, threads=4)
    # two bytes per posting slot of the eligible lists' blocks, inside dir_bytes
    assert on["doc16_bytes"] > 0 and on["doc16_bytes"] % 256 == 0
    assert on["doc16_bytes"] <= 2 * on["impact_bytes"] and on["dir_bytes"] > on["doc16_bytes"]
    saved = os.environ.get("WSR_DOC16")
    os.environ["WSR_DOC16"] = "0"
    try:
        off = w.image_size(d, threads=4)
        assert off["doc16_bytes"] == 0
        assert off["total_bytes"] < on["total_bytes"]
        assert not dc.doc16(d, "d127")[0]
    finally:
        if saved is None:
            os.environ.pop("WSR_DOC16", None)
        else:
            os.environ["WSR_DOC16"] = saved
