"""GPU parity of the lean pipeline's impact-byte pruning (kernels.hip
lean_segment: D bounds a driver posting from its impact byte, and a survivor's
exact driver tf and length code are read by its posting slot when it is
scored), at the smallest shapes where that can go wrong.

Two corpora of 350,000 mostly tiny docs (the doc count is what lets a list of
more than 65 blocks stay below the 2.5 % density of offset buckets).  Every
41st doc holds "ob" (8,537 postings: buckets) and the drivers "d<n>", whose
lists have exactly n postings: 100 (one VInts block), 128 (one pack), 129 (a
pack and a 1-posting VInts tail), 63 and 64 blocks (the edge of a 63-block
item) and 65 blocks.  "om" is in every third doc (a bitmap), "oz" in every
other doc (the third term of the general instance's queries).
  equal:  every driver posting has tf 1 in a doc of one length, and every O1
          posting tf 1: all matches of a query score the same, so every score
          sits exactly at the running threshold and every impact byte is the
          threshold posting's byte;
  varied: tfs 1..3, 254, 255, 256 and 1000 (the 1-byte escape and around it),
          docs from 2 tokens (the corpus' shortest length code) to more than
          a thousand (its longest), few distinct (tf, length) pairs, so ties
          at the threshold stay common.
Everything is compared with the oracle by ==: doc ids, order, f64 scores.
"""
import pytest

from edge_corpora import POSITIONS_HEADER, positions_row

pytestmark = pytest.mark.gpu

N_DOCS = 350_000
STRIDE = 41
SHAPES = (100, 128, 129, 63 * 128, 64 * 128, 65 * 128)
KS = (1, 10, 64)


def _driver_tf(kind, j):
    if kind == "equal":
        return 1
    if j % 500 == 10:
        return 1000
    return {7: 254, 8: 255, 9: 256}.get(j % 50, 1 + j % 3)


def build_impact_index(root, kind):
    import wiser_amd as w
    ld = root / f"{kind}.linedoc"
    with open(ld, "w") as f:
        f.write(POSITIONS_HEADER)
        for i in range(N_DOCS):
            j, r = divmod(i, STRIDE)
            seq = []
            if r == 0:
                parts = [[f"d{n}"] * _driver_tf(kind, j) for n in SHAPES if j < n]
                parts.append(["ob"] * (1 if kind == "equal" else 1 + j % 2))
                # (rotated: which driver stands next to "ob" changes from doc to doc,
                # so two-term phrases occur in some docs and not in others)
                rot = j % len(parts)
                for p in parts[rot:] + parts[:rot]:
                    seq += p
            if i % 3 == 0:
                seq += ["om"] * (1 if kind == "equal" else 1 + i % 2)
            if i % 2 == 0:
                seq.append("oz")
            if r == 0:
                pad = 24 if kind == "equal" else (0, 30)[j % 2]
                seq += [f"f{x}" for x in range(max(0, pad - len(seq)))]
            if not seq:
                seq = ["f0"]
            f.write(positions_row(seq))
    d = root / "idx"
    d.mkdir()
    w.build_from_linedoc(str(ld), str(d), "WITH_POSITIONS")
    return str(d)


class Lab:
    """One index, oracle and engine per corpus; the oracle is asked once per query."""

    def __init__(self, d):
        import wiser_amd as w
        from oracle.oracle import OracleVacuum
        self.dir = d
        self.orc = OracleVacuum(d)
        self.eng = w.VacuumEngine(d, positions=True)
        self.eng.Load()
        self.want = {}

    def expected(self, terms, k, phrase=False):
        key = (tuple(terms), k, phrase)
        if key not in self.want:
            self.want[key] = self.orc.search(list(terms), k, phrase=phrase)[0]
        return self.want[key]

    def run(self, items, k):
        """items: [(terms, phrase)] as one batch -> (launch class, results, stats)"""
        import wiser_amd as w
        from wiser_amd import _capi
        b = w.ResidentBatch(self.eng, len(items), k)
        try:
            b.upload((_capi.Query * len(items))(*[
                self.eng.resolve(w.SearchQuery(list(t), n_results=k, is_phrase=ph))[0] for t, ph in items]))
            cls = b.launch_class()
            b.run()
            hits, nh = b.fetch()
            got = [[(hits[i * k + j].doc_id, hits[i * k + j].score) for j in range(nh[i])]
                   for i in range(len(items))]
            return cls, got, b.stats()
        finally:
            b.close()

    def close(self):
        self.eng.close()
        self.orc.close()


@pytest.fixture(scope="module", params=["equal", "varied"])
def lab(built, tmp_path_factory, request):
    lb = Lab(build_impact_index(tmp_path_factory.mktemp(f"impact_{request.param}"), request.param))
    yield lb
    lb.close()


def two_term():
    """Every driver shape against the bitmap O1 and the bucket O1, the driver
    in slot 0 and in slot 1."""
    qs = []
    for n in SHAPES:
        for o in ("om", "ob"):
            qs += [[f"d{n}", o], [o, f"d{n}"]]
    return qs


def three_term():
    return [[f"d{n}", o, "oz"] for n in SHAPES for o in ("om", "ob")] + [["oz", "ob", f"d{SHAPES[-1]}"]]


def _compare(lab, items, got, k):
    bad = [(t, ph, g[:3], lab.expected(t, k, ph)[:3]) for (t, ph), g in zip(items, got)
           if g != lab.expected(t, k, ph)]
    assert not bad, f"k={k}: {len(bad)}/{len(items)} differ, first: {bad[:3]}"


def test_shapes_are_what_the_cases_need(lab):
    """The lists have the block shapes named above, the drivers are the
    shorter list of every query, and every query has matches."""
    for n in SHAPES:
        assert lab.orc.df(f"d{n}") == n
    assert lab.orc.df("ob") == (N_DOCS + STRIDE - 1) // STRIDE > SHAPES[-1]
    # below / above the 2.5 % density that separates buckets from a bitmap, also per shard
    assert (lab.orc.df("ob") // 2 + 1) * 40 < N_DOCS // 2 and lab.orc.df("om") * 40 >= 2 * N_DOCS
    for q in two_term() + three_term():
        assert lab.expected(q, 1), q


@pytest.mark.parametrize("k", KS)
def test_two_term_instance(lab, k):
    items = [(q, False) for q in two_term()]
    cls, got, st = lab.run(items, k)
    assert cls["two_conj"] and cls["has_conj_lean"] and not cls["has_gen"], cls
    _compare(lab, items, got, k)
    assert st.survivors > 0 and st.driver_blocks >= sum((n + 127) // 128 for n in SHAPES)


@pytest.mark.parametrize("k", KS)
def test_general_lean_instance(lab, k):
    """Three-term queries in the batch: every query runs in the plain lean instance."""
    items = [(q, False) for q in two_term() + three_term()]
    cls, got, _ = lab.run(items, k)
    assert not cls["two_conj"] and cls["has_conj_lean"] and not cls["has_gen"], cls
    _compare(lab, items, got, k)


@pytest.mark.parametrize("k", KS)
def test_two_term_phrase_instance(lab, k):
    items = [(q, True) for q in two_term()]
    cls, got, _ = lab.run(items, k)
    assert cls["has_phrase"] and cls["two_ph"] and not cls["gen_phrase"], cls
    _compare(lab, items, got, k)
    # ("d<n> ob" / "ob d<n>" stand next to each other in some docs)
    assert sum(bool(g) for g in got) >= len(SHAPES)


def test_two_way_doc_range_shards(lab):
    """The same batches over a 2-way doc-range split: the boundary, doc
    175,000, lies inside a block of every list of more than 4,269 postings.
    Three batches per k, as on the full image: two-term queries alone (the
    two-term instance), with three-term queries among them (the plain lean
    instance), and the two-term phrases (the phrase instance)."""
    from test_shard_gpu import _run_step_regions, open_shards
    batches = [(two_term(), False), (two_term() + three_term(), False), (two_term(), True)]
    engs = open_shards(lab.dir, 2, positions=True)
    try:
        for k in KS:
            for qs, phrase in batches:
                qs = qs[:len(qs) // 2 * 2]
                qs2, got = _run_step_regions(lab.dir, qs, k, 2, slot=None, phrase=phrase, engines=engs)
                bad = [(q, g[:3]) for q, g in zip(qs2, got) if g != lab.expected(q, k, phrase)]
                assert not bad, (k, phrase, len(bad), bad[:3])
    finally:
        for e in engs:
            e.close()


def test_survivors_counter_tie_free(built, tmp_path_factory):
    """One small tie-free query through one item: a survivor is a driver
    posting that passed the bound, hit O1 and was scored with its exact tf and
    length code.  The exact check is on the events: at k = 3 they are exactly
    the insertions of the reference heap over the matches in doc order (a wrong
    tf or code of a survivor changes its score, and so the insertions), beside
    the == on the scores.  The survivors counter has no exact value once a
    threshold forms (it is refreshed per chunk): it must lie between the
    insertions and the intersection; with k above the match count no threshold
    ever forms and it is the intersection, whatever the survivors read."""
    import wiser_amd as w
    from wiser_amd import _capi
    from heapmodel import rank_stream
    from oracle.oracle import OracleVacuum
    root = tmp_path_factory.mktemp("impact_tiefree")
    ld = root / "t.linedoc"
    n = 600
    with open(ld, "w") as f:
        f.write(POSITIONS_HEADER)
        for i in range(n):
            seq = ["p"] * (1 + i % 5) + [f"g{x}" for x in range(i % 7)]
            if i % 2 == 0:   # a tf of its own in every doc, in no order (113 and 300 are coprime)
                seq += ["q"] * (1 + ((i // 2) * 113) % 300)
            f.write(positions_row(seq))
    d = root / "idx"
    d.mkdir()
    w.build_from_linedoc(str(ld), str(d), "WITH_POSITIONS")
    orc = OracleVacuum(str(d))
    eng = w.VacuumEngine(str(d), positions=False)
    eng.Load()
    try:
        everything = orc.search(["q", "p"], n)[0]
        assert len(everything) == n // 2
        assert len({s for _, s in everything}) == len(everything)   # tie-free
        in_doc_order = sorted((dc, s) for dc, s in everything)
        for k, exact in ((n, True), (3, False)):
            b = w.ResidentBatch(eng, 1, k)
            try:
                b.upload((_capi.Query * 1)(eng.resolve(w.SearchQuery(["q", "p"], n_results=k))[0]))
                b.run()
                hits, nh = b.fetch()
                got = [(hits[j].doc_id, hits[j].score) for j in range(nh[0])]
                st = b.stats()
                assert got == orc.search(["q", "p"], k)[0]
                assert st.work_items == 1
                if exact:
                    assert st.survivors == len(everything)
                else:
                    _, ins = rank_stream([(s, dc) for dc, s in in_doc_order], k)
                    assert st.events == len(ins), (st.events, len(ins))
                    assert len(ins) <= st.survivors <= len(everything), (st.survivors, len(ins))
            finally:
                b.close()
    finally:
        eng.close()
        orc.close()
