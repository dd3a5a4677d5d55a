"""The skippable-block counter of the conjunctive lean pipeline (kernels.hip
lean_segment: the live driver blocks whose D stage kept no posting,
wsr_batch_stats::skippable_blocks), on a corpus built to
have such blocks, with parity against the oracle by == on every run.

One corpus of 120,000 docs.  Every 41st doc (2,927 of them, 40 tokens long; the
rest have 8) holds "ob" (2.4 % of the docs: offset buckets), "om" and the
drivers; "om" is also in every third doc (a bitmap), "oz" in every other (the
third term of the general instance's queries).  Every driver posting matches
both O1s, so a block's 128 survivors are scored, and the threshold stands, two
iterations after its D.  A driver's postings are "high" (tf 6) or "low" (tf 1)
in docs of one length, so all high matches of a query tie: the threshold
equals the score of every later high posting, whose bound still passes (the
strict > of the reference heap keeps them out later), while a block of low
postings alone passes nothing once k high matches are in.  Per driver, the
kinds of its blocks (H: every third posting high; L: all low; lower case: a
VInts tail block of 50 postings):
  alt    HLHLHLHLHLHL        alternating
  runs   HHLHLLHLLLLLLHLH    runs of 2, 6 (across a floor refresh) and 1
  taill  HLHLHLl             the tail block empty of survivors
  tailh  HLHHLLLh            the tail block not
  head   HLLLLLLLLLL         every block after the first
With items of 3 or 4 blocks (wsr_batch_set_item_blocks) a later item counts
its blocks only where the earlier items' floor has reached it; the items of a
query run at once, so those runs assert parity and the counter's upper bound.
"""
import pytest

from edge_corpora import POSITIONS_HEADER, positions_row

pytestmark = pytest.mark.gpu

N_DOCS = 120_000
STRIDE = 41
DRIVERS = {"alt": "HLHLHLHLHLHL", "runs": "HHLHLLHLLLLLLHLH", "taill": "HLHLHLl", "tailh": "HLHHLLLh",
           "head": "HLLLLLLLLLL"}
TAIL = 50
KS = (1, 10)
WIDE_K = 65   # > kMaxK: every survivor is an event, no threshold, no block without survivors


def n_postings(pat):
    return sum(TAIL if c.islower() else 128 for c in pat)


def _tf(pat, j):
    kind = pat[j // 128]
    return 6 if kind in "Hh" and j % 3 == 0 else 1


def build_index(root):
    import wiser_amd as w
    ld = root / "skip.linedoc"
    with open(ld, "w") as f:
        f.write(POSITIONS_HEADER)
        for i in range(N_DOCS):
            j, r = divmod(i, STRIDE)
            seq = []
            if r == 0:
                parts = [[t] * _tf(pat, j) for t, pat in DRIVERS.items() if j < n_postings(pat)]
                rot = j % (len(parts) + 1)
                parts = parts[rot:] + parts[:rot]   # (which driver stands next to "ob" changes)
                for p in parts:
                    seq += p
                seq.append("ob")
            if i % 3 == 0 or r == 0:
                seq.append("om")
            if i % 2 == 0:
                seq.append("oz")
            want = 40 if r == 0 else 8
            seq += [f"f{x}" for x in range(want - len(seq))]
            f.write(positions_row(seq))
    d = root / "idx"
    d.mkdir()
    w.build_from_linedoc(str(ld), str(d), "WITH_POSITIONS")
    return str(d)


class Lab:
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

    def run(self, items, k, ib=0, eng=None):
        """items: [(terms, phrase)] as one batch -> (launch class, results, stats)"""
        import wiser_amd as w
        from wiser_amd import _capi
        eng = eng or self.eng
        b = w.ResidentBatch(eng, len(items), k)
        try:
            if ib:
                b.set_item_blocks(ib)
            b.upload((_capi.Query * len(items))(*[
                eng.resolve(w.SearchQuery(list(t), n_results=k, is_phrase=ph))[0] for t, ph in items]))
            cls = b.launch_class()
            b.run()
            hits, nh = b.fetch()
            got = [[(hits[i * k + j].doc_id, hits[i * k + j].score) for j in range(nh[i])]
                   for i in range(len(items))]
            return cls, got, b.stats()
        finally:
            b.close()

    def check(self, items, got, k):
        bad = [(t, ph, g[:3], self.expected(t, k, ph)[:3]) for (t, ph), g in zip(items, got)
               if g != self.expected(t, k, ph)]
        assert not bad, f"k={k}: {len(bad)}/{len(items)} differ, first: {bad[:3]}"

    def close(self):
        self.eng.close()
        self.orc.close()


@pytest.fixture(scope="module")
def lab(built, tmp_path_factory):
    lb = Lab(build_index(tmp_path_factory.mktemp("blockskip")))
    yield lb
    lb.close()


def two_term(o):
    """Every driver against one O1, the driver in slot 0 and in slot 1."""
    qs = []
    for t in DRIVERS:
        qs += [[t, o], [o, t]]
    return qs


def test_shapes_are_what_the_cases_need(lab):
    for t, pat in DRIVERS.items():
        assert lab.orc.df(t) == n_postings(pat)
    ob = lab.orc.df("ob")
    assert ob == (N_DOCS + STRIDE - 1) // STRIDE > max(map(n_postings, DRIVERS.values()))
    # below / above the 2.5 % density that separates buckets from a bitmap, also per shard
    assert (ob // 2 + 1) * 40 < N_DOCS // 2 and lab.orc.df("om") * 40 >= 2 * N_DOCS
    for t in DRIVERS:   # more high matches in the first block than the largest pruning k
        assert len(lab.expected([t, "om"], 10)) == 10


@pytest.mark.parametrize("ib", (0, 3, 4))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("o1", ("om", "ob"))
def test_two_term_instance_counts(lab, o1, k, ib):
    """The bitmap copy (om) and the bucket copy (ob): each driver alone in its
    batch, so that the counter is its own."""
    for t in DRIVERS:
        items = [([t, o1], False), ([o1, t], False)]
        cls, got, st = lab.run(items, k, ib)
        assert cls["two_conj"] and cls["has_conj_lean"] and not cls["has_gen"], cls
        lab.check(items, got, k)
        n_blk = len(DRIVERS[t])
        assert st.driver_blocks <= 2 * n_blk
        # only blocks with no high posting can be empty; in a one-item query
        # every driver has such blocks past the point where the threshold stands
        assert st.skippable_blocks <= 2 * DRIVERS[t].upper().count("L"), (t, o1, k, ib, st.skippable_blocks)
        if ib == 0:
            assert st.skippable_blocks > 0, (t, o1, k)


@pytest.mark.parametrize("ib", (0, 3))
@pytest.mark.parametrize("k", KS)
def test_general_lean_instance_counts(lab, k, ib):
    """Three-term queries in the batch: every query runs in the plain lean instance."""
    items = [(q, False) for q in two_term("om") + two_term("ob")]
    items += [([t, o, "oz"], False) for t in DRIVERS for o in ("om", "ob")] + [(["oz", "ob", "runs"], False)]
    cls, got, st = lab.run(items, k, ib)
    assert not cls["two_conj"] and cls["has_conj_lean"] and not cls["has_gen"], cls
    lab.check(items, got, k)
    if ib == 0:
        assert st.skippable_blocks > 0


@pytest.mark.parametrize("ib", (0, 3))
def test_wide_counts_none(lab, ib):
    items = [(q, False) for q in two_term("om") + two_term("ob")] + [(["runs", "om", "oz"], False)]
    cls, got, st = lab.run(items, WIDE_K, ib)
    assert cls["has_conj_lean"] and not cls["has_gen"], cls
    lab.check(items, got, WIDE_K)
    assert st.skippable_blocks == 0
    assert st.driver_blocks > 0


@pytest.mark.parametrize("k", KS + (WIDE_K,))
def test_two_term_phrase_instance_counts_none(lab, k):
    """The phrase instances do not prune on impact bytes: their counter reads 0."""
    items = [(q, True) for q in two_term("ob")]
    cls, got, st = lab.run(items, k)
    # (k > kMaxK: the phrase queries leave the two-term phrase class)
    assert cls["has_phrase"] and (cls["two_ph"] and not cls["gen_phrase"] or k == WIDE_K), cls
    lab.check(items, got, k)
    assert any(got)   # (a driver stands next to "ob" in some docs)
    assert st.skippable_blocks == 0


def test_two_way_doc_range_shards(lab):
    """A 2-way doc-range split (the boundary, doc 60,000, lies inside a block of
    every driver of more than 1,464 postings): parity of the exchange's result,
    and the counter on a shard's own image."""
    from test_shard_gpu import _run_step_regions, open_shards
    engs = open_shards(lab.dir, 2, positions=True)
    try:
        for k in KS + (WIDE_K,):
            qs = two_term("om") + two_term("ob")
            qs2, got = _run_step_regions(lab.dir, qs, k, 2, slot=None, phrase=False, engines=engs)
            bad = [(q, g[:3]) for q, g in zip(qs2, got) if g != lab.expected(q, k, False)]
            assert not bad, (k, len(bad), bad[:3])
        _, _, st = lab.run([(q, False) for q in two_term("om")], 10, eng=engs[0])
        assert st.skippable_blocks > 0
        # wide items count none on either shard: a boundary block's postings of
        # the other half are out of range, not postings that failed the bound
        for e in engs:
            _, _, st = lab.run([(q, False) for q in two_term("om") + two_term("ob")], WIDE_K, eng=e)
            assert st.driver_blocks > 0 and st.skippable_blocks == 0
    finally:
        for e in engs:
            e.close()
