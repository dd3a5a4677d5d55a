"""CPU: the stair corpus (stair_corpus.py) and the window-schedule model
(window_model.py), from the writer and the oracle alone.  Every assertion here
is a condition the corpus was chosen to meet, so that the exact-counter checks
of test_gpu_maxscore.py are not vacuous: the essential set shrinks in stages,
windows are skipped in each stage, each match rule loses hits while skipping
goes on, filters pass windows over, a run window lies past doc 65,535, every
exact-counter query is one work item, and a wrong bound order or a duplicate
slot counted once gives another schedule."""
import pytest

import stair_corpus as sc
import window_model as wm
from bool_model import BoolModel
from heapmodel import rank_stream
from or_model import OrModel

M, S, N = "must", "should", "must_not"
KS = (1, 10, 64)


def q(text, min_should=0):
    """'+a b -c' -> ([(a, must), (b, should), (c, must_not)], min_should)"""
    terms = []
    for t in text.split():
        terms.append((t[1:], M) if t[0] == "+" else (t[1:], N) if t[0] == "-" else (t, S))
    return terms, min_should


OR_QUERIES = (["lo mid hi", "lo hi mid", "mid lo hi", "mid hi lo", "hi lo mid", "hi mid lo"] +
              ["lo lo hi", "hi lo lo", "lo lo2 mid hi"])
BOOL_QUERIES = [q("lo mid hi", 1), q("lo mid hi", 2), q("lo mid hi -ban"), q("+hi lo mid")]
# the complement of a window-aligned range; docs of hi-free windows only
FILTERS = {
    "outside_3_10": set(range(sc.N_DOCS)) - set(range(3 * sc.WINDOW, 10 * sc.WINDOW)),
    "hi_free": {d for w in (1, 3, 20, 34) for d in range(w * sc.WINDOW, (w + 1) * sc.WINDOW) if d % 3 == 1},
}
SHARDS = [(0, sc.SHARD_CUTS[0]), (sc.SHARD_CUTS[0], sc.SHARD_CUTS[1]), (sc.SHARD_CUTS[1], sc.N_DOCS)]


class StairModel:
    """The models of one index: contributions (OrModel), matches (BoolModel)
    and window schedules (window_model.walk), shared and computed once."""

    def __init__(self, orc):
        from oracle.oracle import lib
        self.orc = orc
        self.om = OrModel(orc)
        self.bm = BoolModel(self.om)
        self.n_docs = orc.n_docs()
        self.idf = lambda t: lib.orc_es_idf(self.n_docs, orc.df(t))
        self._posts, self._sched = {}, {}

    def postings(self, t):
        if t not in self._posts:
            self._posts[t] = sorted(self.om.contrib(t))
        return self._posts[t]

    def blocks(self, terms):
        return sum((len(self.postings(t)) + wm.BLOCK - 1) // wm.BLOCK for t, _ in terms)

    def item(self, terms, doc_range=None, whole_lists=False):
        """The kept slots of the query in the image of doc_range (a slot whose
        list has no block there is dropped) and its one item's doc range.
        whole_lists: doc_range is an item of the whole index's image, not a shard."""
        lo, hi = doc_range or (0, self.n_docs)
        kept = [(t, r, wm.list_end(self.postings(t), *((0, None) if whole_lists else (lo, hi)))) for t, r in terms]
        kept = [x for x in kept if x[2] > 0]
        return kept, lo, min(hi, max(e for _, _, e in kept))

    def schedule(self, terms, ms, k, doc_range=None, filter_name=None, **variant):
        """variant: skipping=False, order="query", dup_once=True (window_model.walk)"""
        key = (tuple(terms), ms, k, doc_range, filter_name, tuple(sorted(variant.items())))
        if key not in self._sched:
            docset = FILTERS[filter_name] if filter_name is not None else None
            kept, lo, hi = self.item(terms, doc_range, variant.pop("whole_lists", False))
            if docset:   # (a filtered query's items are cut to the set's first and last doc)
                lo = max(lo, min(docset))
                hi = max(lo, min(hi, max(docset) + 1))
            names = [t for t, _, _ in kept] if variant.pop("dup_once", False) else None
            self._sched[key] = wm.walk([self.om.contrib(t) for t, _, _ in kept], [r for _, r, _ in kept],
                                       [2.2 * self.idf(t) for t, _, _ in kept], k, lo, hi, ms, docset,
                                       [e for _, _, e in kept], names=names, **variant)
        return self._sched[key]

    def items(self, terms, target):
        """The work items of the query over the whole index: its doc range cut
        at the last doc of every s-th block of its longest list, s = target x
        blocks(longest) / blocks(all lists), at least 1 ("Plan")."""
        kept, lo, hi = self.item(terms)
        nblk = [(len(self.postings(t)) + wm.BLOCK - 1) // wm.BLOCK for t, _, _ in kept]
        g = self.postings(kept[nblk.index(max(nblk))][0])
        step = max(1, target * max(nblk) // sum(nblk))
        cuts = [lo] + [g[j * wm.BLOCK - 1] + 1 for j in range(step, max(nblk), step)] + [hi]
        return [(a, b) for a, b in zip(cuts, cuts[1:]) if a < b]

    def schedules(self, terms, ms, k, target, **variant):
        """One Schedule per work item: every item starts with a full essential set."""
        return [self.schedule(terms, ms, k, doc_range=rg, whole_lists=True, **variant)
                for rg in self.items(terms, target)]

    def stream(self, terms, ms, doc_range=None, docset=None):
        return [(s, d) for s, d in self.bm.matching(terms, ms, doc_range) if docset is None or d in docset]


def or_terms(text):
    return [(t, S) for t in text.split()]


@pytest.fixture(scope="module")
def stair(built, tmp_path_factory):
    from oracle.oracle import OracleVacuum
    d = sc.build_stair_index(tmp_path_factory.mktemp("stair"))
    orc = OracleVacuum(d)
    yield StairModel(orc)
    orc.close()


def test_corpus_shape(stair):
    df = {t: stair.orc.df(t) for t in ("hi", "mid", "lo", "lo2", "ban")}
    assert stair.n_docs == sc.N_DOCS == 73728
    assert df["hi"] == 48 and 300 <= df["mid"] <= 640 and df["lo"] <= 31 * 128 and df["lo2"] <= 25 * 128, df
    assert df["lo"] >= 3500 and df["lo2"] >= 3000 and df["ban"] > 0
    win = {t: {d // sc.WINDOW for d in stair.postings(t)} for t in df}
    assert win["hi"] == set(sc.HI_WINDOWS) and max(stair.postings("hi")) > 65535
    for g in (sc.G1, sc.G2, sc.G3):
        assert len(g) >= 12 and set(g) <= set(stair.postings("hi"))
        assert set(g) & set(stair.postings("ban")) and set(g) - set(stair.postings("ban"))
    everywhere = set(range(sc.N_WINDOWS)) - set(sc.EMPTY_WINDOWS)
    assert win["lo"] == win["lo2"] == everywhere
    assert not any(w in win[t] for t in df for w in sc.EMPTY_WINDOWS)
    assert len(everywhere - win["hi"] - win["mid"]) >= 6
    assert {d % sc.WINDOW for d in stair.postings("mid")} >= {0, 1, 2047}
    assert win["mid"] - win["hi"] and win["mid"] & win["hi"]
    lo_only = set(stair.postings("lo")) - set(stair.postings("hi")) - set(stair.postings("mid"))
    assert lo_only & set(stair.postings("ban"))
    assert len({s for s in stair.om.contrib("lo").values()}) >= 8   # (tfs 1-3, four lengths)
    # the bounds: hi alone lies between twice lo's and lo's + mid's
    ub = {t: 2.2 * stair.idf(t) for t in df}
    assert ub["lo"] < ub["lo2"] < ub["mid"] < ub["hi"] and 2 * ub["lo"] < ub["hi"] < ub["lo"] + ub["mid"]
    assert all(s < ub[t] for t in ("hi", "mid", "lo", "lo2") for s in stair.om.contrib(t).values())


def test_exact_counter_queries_are_one_item(stair):
    for text in OR_QUERIES:
        assert stair.blocks(or_terms(text)) <= 63, text
    for t, _ in BOOL_QUERIES:
        assert stair.blocks(t) <= 63, t


def test_stages_of_three_tiers(stair):
    """[lo, mid, hi] at k = 10: 3 -> 2 -> 1 within the one item, with windows
    skipped in the 2-stage and in the 1-stage, and a run window past 65,535."""
    for text in OR_QUERIES[:6]:
        terms = or_terms(text)
        s = stair.schedule(terms, 0, 10)
        assert s.stages == [3, 2, 1], (text, s.stages)
        # replay with the skip count split per stage
        two = stair.schedule(terms, 0, 10, doc_range=(0, sc.HI_WINDOWS[1] * sc.WINDOW))
        assert two.stages == [3, 2] and 0 < two.skipped < s.skipped, (two.stages, two.skipped, s.skipped)
        assert max(s.run_bases) > 65535
        full = stair.schedule(terms, 0, 10, skipping=False)
        assert s.windows < full.windows == sc.N_WINDOWS - len(sc.EMPTY_WINDOWS) and full.skipped == 0
        # exactness: the docs in skipped windows are never insertions
        assert s.events == full.events == len(rank_stream(stair.stream(terms, 0), 10)[1])
        assert rank_stream(s.stream, 10)[0] == stair.om.expected(text.split(), 10)
    # all six orders walk the same windows
    assert len({tuple(stair.schedule(or_terms(t), 0, 10).run_bases) for t in OR_QUERIES[:6]}) == 1


def test_duplicate_slots_leave_together(stair):
    for text in ("lo lo hi", "hi lo lo"):
        s = stair.schedule(or_terms(text), 0, 10)
        assert s.stages == [3, 1] and s.skipped > 0, (text, s.stages, s.skipped)
    # at k = 64 the threshold stays between one lo bound and two: one slot leaves alone
    assert stair.schedule(or_terms("lo lo hi"), 0, 64).stages == [3, 2]


def test_four_tiers(stair):
    s = stair.schedule(or_terms("lo lo2 mid hi"), 0, 10)
    # (hi with mid stays below lo's + lo2's + mid's bound: mid is essential to the end)
    assert s.stages == [4, 3, 2] and s.skipped > 0, s.stages


def test_bool_rules_lose_hits_while_skipping(stair):
    for k in KS:
        two = stair.schedule(*q("lo mid hi", 2), k)
        ban = stair.schedule(*q("lo mid hi -ban"), k)
        assert two.skipped > 0 and ban.skipped > 0, (k, two.skipped, ban.skipped)
    assert stair.bm.explain(*q("lo mid hi", 2)).lost_should > 0
    assert stair.bm.explain(*q("lo mid hi -ban")).lost_not > 0
    # a hit of the unrestricted top-64 (every doc with hi) is lost to each rule
    top = {d for _, d in stair.bm.expected(q("lo mid hi")[0], 64)}
    assert top - {d for _, d in stair.bm.matching(*q("lo mid hi", 2))}
    assert top - {d for _, d in stair.bm.matching(*q("lo mid hi -ban"))}
    # MUST_NOT postings are touched in every run window: some run window holds a doc with ban alone
    ban = stair.schedule(*q("lo mid hi -ban"), 64)
    in_run = {t: {d for d in stair.postings(t) if d - d % sc.WINDOW in ban.run_bases} for t in ("lo", "mid", "hi", "ban")}
    scored = in_run["lo"] | in_run["mid"] | in_run["hi"]
    assert ban.touched == len(scored | in_run["ban"]) > len(scored)
    # a MUST lead: no skipping, and only the windows that hold hi run
    led = stair.schedule(*q("+hi lo mid"), 10)
    assert led.skipped == 0 and led.stages == [1] and led.run_bases == [w * sc.WINDOW for w in sc.HI_WINDOWS]


def test_filters_run_and_pass_windows(stair):
    hi_windows = {d // sc.WINDOW for d in stair.postings("hi")}
    assert not {d // sc.WINDOW for d in FILTERS["hi_free"]} & hi_windows
    for name in FILTERS:
        for terms, ms in BOOL_QUERIES[:3]:
            s = stair.schedule(terms, ms, 10, filter_name=name)
            assert s.windows > 0 and s.passed > 0 and s.skipped > 0, (name, terms, ms, s[:3])
            assert rank_stream(s.stream, 10)[0] == rank_stream(stair.stream(terms, ms, None, FILTERS[name]), 10)[0]


def test_shards_restart_full(stair):
    """Each doc-range shard is an item of its own: the essential set starts
    full again, and the shards' schedules are not the whole index's cut up."""
    terms = or_terms("lo mid hi")
    whole = stair.schedule(terms, 0, 10)
    parts = [stair.schedule(terms, 0, 10, doc_range=rg) for rg in SHARDS]
    assert all(p.stages[0] == 3 and p.windows > 0 for p in parts)
    assert sum(p.windows for p in parts) > whole.windows
    assert any(p.skipped > 0 for p in parts)
    assert sc.G2[0] < SHARDS[0][1] <= sc.G2[-1] and SHARDS[1][1] == 36864


def test_items_restart_full(stair):
    """Shorter items (DESIGN 4j's cut at the longest list's blocks): every
    item starts with all its slots essential, so the windows run grow as the
    items shrink, and some item still skips."""
    terms = or_terms("lo mid hi")
    one = stair.schedule(terms, 0, 10)
    assert stair.items(terms, 63) == [(0, max(stair.postings("lo")) + 1)]
    seen = one.windows
    for target in (8, 1):
        parts = stair.schedules(terms, 0, 10, target)
        assert len(parts) > 1 and all(p.stages[0] == 3 for p in parts if p.windows)
        assert sum(p.skipped for p in parts) > 0, target
        full = sum(p.windows for p in stair.schedules(terms, 0, 10, target, skipping=False))
        assert seen < sum(p.windows for p in parts) <= full
        seen = sum(p.windows for p in parts)
    assert len(stair.items(terms, 1)) == 31


def test_wrong_models_differ(stair):
    """Bounds summed in query order, or a repeated term's bound counted once,
    walk another schedule on some case: the cases tell such a kernel apart."""
    def key(s):
        return (s.windows, s.skipped, s.touched, s.events, tuple(s.stages))
    cases = [(or_terms(t), 0, k) for t in OR_QUERIES for k in KS]
    assert any(key(stair.schedule(t, ms, k)) != key(stair.schedule(t, ms, k, order="query")) for t, ms, k in cases)
    dups = [(or_terms(t), 0, k) for t in ("lo lo hi", "hi lo lo") for k in KS]
    assert any(key(stair.schedule(t, ms, k)) != key(stair.schedule(t, ms, k, dup_once=True)) for t, ms, k in dups)
