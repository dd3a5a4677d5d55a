"""The lean pipeline's 16-bit doc id copy (kernels.hip lean_segment kD16: W
loads one dword of doc16 per lane, D forms a0 and a1 with one add each) against
the oracle by == on the whole index, with the array on and with WSR_DOC16=0
(every driver's packs unpacked), on the hand-made corpus of doc16_corpus.py and
the tie and random corpora of edge_corpora.py.

The corpus has 680,000 docs, not a few tens of thousands: a bucket O1 is no
shorter than its driver and below 2.5 % density, so the 127-block driver's
needs more than 650,240 docs (doc16_corpus.py).  Its docs hold a few tokens, so
the index is built and loaded in seconds.

Every case asserts from the launch class and the batch statistics that
conjunctive lean items ran, and the module asserts from image_info and the
accessor (wsr_debug_doc16) that the drivers meant to be eligible are, so that
no case passes on the unpack path alone.
"""
import os
from contextlib import contextmanager

import pytest

import doc16_corpus as dc

pytestmark = pytest.mark.gpu

DRIVERS = ("d2t", "d63", "d64", "d127")
ELIGIBLE = DRIVERS + ("s", "f", "p", "ob")
INELIGIBLE = ("t", "q")


@contextmanager
def doc16_env(on):
    saved = os.environ.get("WSR_DOC16")
    if on:
        os.environ.pop("WSR_DOC16", None)
    else:
        os.environ["WSR_DOC16"] = "0"
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("WSR_DOC16", None)
        else:
            os.environ["WSR_DOC16"] = saved


class Lab:
    """One index: its oracle, an engine with the array and one without."""

    def __init__(self, d, positions=False):
        import wiser_amd as w
        from oracle.oracle import OracleVacuum
        self.dir = d
        self.orc = OracleVacuum(d)
        self.eng = {}
        for on in (True, False):
            with doc16_env(on):
                e = w.VacuumEngine(d, positions=positions)
                e.Load()
            self.eng[on] = e
        self.want = {}

    def expected(self, terms, k):
        key = (tuple(terms), k)
        if key not in self.want:
            self.want[key] = self.orc.search(list(terms), k)[0]
        return self.want[key]

    def run(self, eng, queries, k, ib=0):
        """queries as one batch -> (launch class, results, stats)"""
        import wiser_amd as w
        from wiser_amd import _capi
        b = w.ResidentBatch(eng, len(queries), k)
        try:
            if ib:
                b.set_item_blocks(ib)
            b.upload((_capi.Query * len(queries))(*[
                eng.resolve(w.SearchQuery(list(t), n_results=k))[0] for t in queries]))
            cls = b.launch_class()
            b.run()
            hits, nh = b.fetch()
            got = [[(hits[i * k + j].doc_id, hits[i * k + j].score) for j in range(nh[i])]
                   for i in range(len(queries))]
            return cls, got, b.stats()
        finally:
            b.close()

    def check(self, queries, k, ib=0, two=True, all_lean=True):
        """Parity on the engine with the array and on the one without; lean items ran."""
        for on, eng in self.eng.items():
            cls, got, st = self.run(eng, queries, k, ib)
            assert cls["has_conj_lean"] and bool(cls["two_conj"]) == two, (on, cls)
            assert not (all_lean and cls["has_gen"]), (on, cls)
            assert st.driver_blocks > 0, on
            bad = [(q, g[:3], self.expected(q, k)[:3]) for q, g in zip(queries, got) if g != self.expected(q, k)]
            assert not bad, f"doc16 {'on' if on else 'off'} k={k} ib={ib}: {len(bad)}/{len(queries)} differ: {bad[:3]}"

    def close(self):
        for e in self.eng.values():
            e.close()
        self.orc.close()


@pytest.fixture(scope="module")
def lab(built, tmp_path_factory):
    lb = Lab(dc.build_index(tmp_path_factory.mktemp("doc16gpu")))
    yield lb
    lb.close()


@pytest.fixture(scope="module")
def ties(built, tmp_path_factory):
    from edge_corpora import build_tie_index
    lb = Lab(build_tie_index(tmp_path_factory.mktemp("doc16ties")))
    yield lb
    lb.close()


def both_orders(pairs):
    return [list(p) for a, b in pairs for p in ((a, b), (b, a))]


def test_the_drivers_meant_to_be_eligible_are(lab, ties):
    on, off = lab.eng[True].image_info(), lab.eng[False].image_info()
    assert on["doc16_bytes"] > 0 and off["doc16_bytes"] == 0
    assert on["total_bytes"] - off["total_bytes"] >= on["doc16_bytes"]
    for t in ELIGIBLE:
        assert dc.doc16(lab.dir, t, max_blocks=1)[0], t
    for t in INELIGIBLE:
        assert not dc.doc16(lab.dir, t, max_blocks=1)[0], t
    for t, n in (("d2t", 3), ("d63", 63), ("d64", 64), ("d127", 127)):
        assert dc.doc16(lab.dir, t, max_blocks=1)[1] == n == (lab.orc.df(t) + 127) // 128
    # every driver is shorter than both O1s; in the image ob has offset buckets and z a rank bitmap
    assert 127 < (lab.orc.df("ob") + 127) // 128 < (lab.orc.df("z") + 127) // 128
    assert dc.doc16_probe(lab.dir, "ob")[4] >= 3 and dc.doc16_probe(lab.dir, "z")[4] == 0
    assert ties.eng[True].image_info()["doc16_bytes"] > 0
    for t in "abcd":
        assert dc.doc16(ties.dir, t, max_blocks=1)[0], t


@pytest.mark.parametrize("ib", (0, 1, 7))
@pytest.mark.parametrize("o1", ("z", "ob"))
def test_item_edges(lab, o1, ib):
    """Drivers of 2 pack blocks + tail, 63, 64 and 127 blocks against a bitmap
    O1 (z) and a bucket O1 (ob); whole-list items, one-block items, 7-block items."""
    lab.check(both_orders((t, o1) for t in DRIVERS), 10, ib)


def test_eligible_and_ineligible_drivers_in_one_launch(lab):
    qs = both_orders([("d64", "z"), ("t", "z"), ("s", "ob"), ("q", "z"), ("t", "ob"), ("d2t", "ob"), ("g", "z"),
                      ("p", "z"), ("f", "z")])
    lab.check(qs, 10)
    lab.check(qs, 1, ib=2)


def test_last_posting_at_offset_0xffff(lab):
    edge = dc.lists()["s"][255]
    for k in (10, 64):
        want = lab.expected(["s", "z"], k)
        assert edge in [d for d, _ in want], k   # the posting at the edge is a result
        lab.check([["s", "z"], ["z", "s"], ["t", "z"]], k)


@pytest.mark.parametrize("ib", (0, 1, 3))
@pytest.mark.parametrize("k", (1, 10))
def test_ties_at_block_edges(ties, k, ib):
    """Scores that tie with the threshold (the reference heap's strict >), with
    the threshold handed on at every block edge (one-block items) and inside
    longer items."""
    ties.check(both_orders([("b", "a"), ("c", "a"), ("d", "a"), ("c", "b"), ("d", "b"), ("d", "c")]), k, ib)


def test_three_term_queries_run_the_general_instance(lab):
    qs = [["d64", "ob", "z"], ["z", "d2t", "ob"], ["s", "z", "ob"], ["d127", "z"], ["t", "z", "ob"]]
    lab.check(qs, 10, two=False)
    lab.check(qs, 10, ib=5, two=False)


def _sharded(lab_, index_dir, ranges, queries, k):
    """The exchange's results over the doc-range shards `ranges`, array on and
    off, against the oracle; and each shard's own launch runs lean items."""
    from test_shard_gpu import _run_step_regions, open_shards
    world = len(ranges)
    assert len(queries) % world == 0
    for on in (True, False):
        with doc16_env(on):
            engs = open_shards(index_dir, world, ranges=ranges)
        try:
            assert (engs[0].image_info()["doc16_bytes"] > 0) == on
            qs2, got = _run_step_regions(index_dir, queries, k, world, slot=None, engines=engs)
            bad = [(q, g[:3]) for q, g in zip(qs2, got) if g != lab_.expected(q, k)]
            assert not bad, (on, k, len(bad), bad[:3])
            ran = [lab_.run(e, queries, k) for e in engs]
            assert any(cls["has_conj_lean"] and st.driver_blocks > 0 for cls, _, st in ran), on
        finally:
            for e in engs:
                e.close()


def test_two_way_split_inside_a_driver_block(lab):
    ids = dc.lists()["d127"]
    cut = dc.N_DOCS // 2
    b = next(b for b in range(127) if ids[128 * b + 127] >= cut)
    assert ids[128 * b] < cut <= ids[128 * b + 127]   # the cut falls inside block b
    assert dc.doc16(lab.dir, "d127", (cut, dc.N_DOCS), max_blocks=1)[:2] == (True, 127 - b)
    qs = both_orders([("d127", "z"), ("d127", "ob"), ("d64", "z"), ("d63", "ob")])
    for k in (1, 10):
        _sharded(lab, lab.dir, [(0, cut), (cut, dc.N_DOCS)], qs, k)


def test_shard_inside_a_posting_gap(built, tmp_path_factory):
    """The rand1 gap cut of test_gpu_shard_instances.py: the middle shard lies
    between two neighbouring postings of one of x127 / x128 / x129, so its
    image holds a block of that list and none of its postings."""
    from edge_corpora import build_skewed_index
    from test_gpu_shard_instances import GAP_LISTS, image_blocks, widest_gap_cut
    d, _ = build_skewed_index(tmp_path_factory.mktemp("doc16rand1"), 1)
    lb = Lab(d)
    try:
        t, rgs = widest_gap_cut(lb.orc, lb.orc.n_docs())
        docs = lb.orc.postings(t)[0]
        lo, hi = rgs[1]
        assert lo < hi and image_blocks(docs, lo, hi) and not any(lo <= x < hi for x in docs)
        assert lb.eng[True].image_info()["doc16_bytes"] > 0
        assert any(dc.doc16(d, x, max_blocks=1)[0] for x in GAP_LISTS)
        qs = both_orders([(x, "v0") for x in GAP_LISTS]) + [["x256", "v0"], ["x300", "v0"], ["v0", "x255"]]
        assert len(qs) % 3 == 0
        lb.check(qs, 10, all_lean=False)
        for k in (1, 10):
            _sharded(lb, d, [tuple(r) for r in rgs], qs, k)
    finally:
        lb.close()
