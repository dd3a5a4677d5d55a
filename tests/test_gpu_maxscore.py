"""GPU: the MaxScore window skipping of the windowed traversal (kernels.hip
window_item: or_kernel, bool_kernel, bool_filtered_kernel) on the stair corpus
(stair_corpus.py).  Results are compared with == against OrModel / BoolModel:
doc ids, order and f64 scores, no tolerance.  The schedule counters of
wsr_or_stats -- windows, windows_skipped, touched_docs, events -- must equal
the window model's (window_model.py, written from DESIGN 4j / 4l / 4o), per
work item and summed; test_window_model.py shows on the CPU that the cases
reach every stage of the rule."""
import pytest

import stair_corpus as sc
from heapmodel import rank_stream
from test_gpu_bool import run_bool
from test_gpu_count import run_count as run_count_ex
from test_gpu_docset import match_set, run_count, run_search
from test_window_model import BOOL_QUERIES, FILTERS, KS, OR_QUERIES, SHARDS, StairModel, or_terms

pytestmark = pytest.mark.gpu

COUNTERS = ("windows", "windows_skipped", "touched_docs", "events")


class _Stair:
    def __init__(self, d):
        import wiser_amd as w
        from oracle.oracle import OracleVacuum
        self.dir = d
        self.eng = w.VacuumEngine(d, positions=False)
        self.eng.Load()
        self.orc = OracleVacuum(d)
        self.sm = StairModel(self.orc)
        self.sets = {name: self.eng.docset(sorted(ids)) for name, ids in FILTERS.items()}

    def close(self):
        for s in self.sets.values():
            s.close()
        self.eng.close()
        self.orc.close()


@pytest.fixture(scope="module")
def stair(built, tmp_path_factory):
    c = _Stair(sc.build_stair_index(tmp_path_factory.mktemp("stair_gpu")))
    yield c
    c.close()


def run_or(eng, terms, k, item_blocks=None):
    """One WSR_QUERY_OR query in a resident batch of its own -> ([(score, doc)], wsr_or_stats)"""
    import wiser_amd as w
    from wiser_amd import _capi
    b = w.ResidentBatch(eng, 1, k)
    try:
        if item_blocks is not None:
            b.set_item_blocks(item_blocks)
        b.upload((_capi.Query * 1)(eng.resolve(w.SearchQuery(list(terms), n_results=k, match_any=True))[0]))
        b.run()
        hits, nh = b.fetch()
        return [(hits[j].score, hits[j].doc_id) for j in range(nh[0])], b.or_stats()
    finally:
        b.close()


def counters(st):
    return tuple(getattr(st, f) for f in COUNTERS)


def summed(parts):
    """the four counters of a list of window_model.Schedule, in COUNTERS' order"""
    return (sum(p.windows for p in parts), sum(p.skipped for p in parts), sum(p.touched for p in parts),
            sum(p.events for p in parts))


# ---- one item: all four counters ---------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_or_exact_counters(stair, k):
    sm = stair.sm
    for text in OR_QUERIES:
        got, st = run_or(stair.eng, text.split(), k)
        assert got == sm.om.expected(text.split(), k) and len(got) == k, (text, k)
        assert st.items == 1, (text, st.items)
        assert counters(st) == summed([sm.schedule(or_terms(text), 0, k)]), (text, k)


@pytest.mark.parametrize("k", KS)
def test_bool_exact_counters(stair, k):
    sm = stair.sm
    hi_windows = len({d // sc.WINDOW for d in sm.postings("hi")})
    for terms, ms in BOOL_QUERIES:
        for name in (None,) + tuple(FILTERS):
            ids = FILTERS[name] if name else None
            if name:
                (got,), st = run_search(stair.eng, [(terms, ms, k)], [stair.sets[name]])
            else:
                (got,), st = run_bool(stair.eng, [(terms, ms, k)])
            want = rank_stream(sm.stream(terms, ms, None, ids), k)[0]
            assert got == want, (terms, ms, k, name, got[:3], want[:3])
            model = sm.schedule(terms, ms, k, filter_name=name)
            if model.windows == 0:   # (a lead with no doc in the set: nothing runs)
                assert counters(st) == (0, 0, 0, 0) and got == []
                continue
            assert st.items == 1, (terms, st.items)
            assert counters(st) == summed([model]), (terms, ms, k, name)
            if terms[0][1] == "must":
                assert 0 < st.windows <= hi_windows and st.windows_skipped == 0


def test_wide_k_never_skips(stair):
    """k = 65: every matching doc is an event and no window is skipped."""
    sm = stair.sm
    for text in OR_QUERIES:
        got, st = run_or(stair.eng, text.split(), 65)
        assert got == sm.om.expected(text.split(), 65)
        assert st.windows_skipped == 0 and st.events == len(sm.stream(or_terms(text), 0)), text
        assert counters(st) == summed([sm.schedule(or_terms(text), 0, 65)]), text
    for terms, ms in BOOL_QUERIES:
        (got,), st = run_bool(stair.eng, [(terms, ms, 65)])
        assert got == sm.bm.expected(terms, 65, ms)
        assert st.windows_skipped == 0 and st.events == len(sm.stream(terms, ms)), (terms, ms)
        assert counters(st) == summed([sm.schedule(terms, ms, 65)]), (terms, ms)


# ---- item edges ------------------------------------------------------------------------
@pytest.mark.parametrize("item_blocks", [63, 8, 1])
def test_item_edges(stair, item_blocks):
    """Every item starts with a full essential set: the counters are the sum
    of the model walked item by item, at most the windows it runs without
    skipping, and some item still skips."""
    sm = stair.sm
    skipped = 0
    for k in KS:
        cases = [(or_terms(t), 0, True) for t in OR_QUERIES] + [(t, ms, False) for t, ms in BOOL_QUERIES]
        for terms, ms, as_or in cases:
            if as_or:
                got, st = run_or(stair.eng, [t for t, _ in terms], k, item_blocks)
            else:
                (got,), st = run_bool(stair.eng, [(terms, ms, k)], item_blocks)
            assert got == sm.bm.expected(terms, k, ms), (terms, ms, k, item_blocks)
            parts = sm.schedules(terms, ms, k, item_blocks)
            full = sm.schedules(terms, ms, k, item_blocks, skipping=False)
            assert st.windows <= sum(p.windows for p in full), (terms, ms, k)
            if terms[0][1] != "must":   # (a led query drops the items without a lead block)
                assert st.items == len(parts), (terms, ms, k, st.items, len(parts))
            assert counters(st) == summed(parts), (terms, ms, k, item_blocks)
            skipped += st.windows_skipped
    assert skipped > 0


# ---- doc-range shards --------------------------------------------------------------------
@pytest.mark.parametrize("rg", SHARDS, ids=lambda rg: f"{rg[0]}-{rg[1]}")
def test_shard_edges(stair, rg):
    """A shard's answer is the model restricted to its docs; its one item
    starts with a full essential set, whatever the shard before it reached."""
    import wiser_amd as w
    sm = stair.sm
    eng = w.VacuumEngine(stair.dir, doc_range=rg, positions=False)
    eng.Load()
    try:
        some = 0
        for k in KS:
            for text in OR_QUERIES:
                got, st = run_or(eng, text.split(), k)
                want = rank_stream(sm.stream(or_terms(text), 0, rg), k)[0]
                assert got == want, (rg, text, k, got[:3], want[:3])
                assert st.items == 1 and counters(st) == summed([sm.schedule(or_terms(text), 0, k, doc_range=rg)]), \
                    (rg, text, k)
                some += len(got)
            for terms, ms in BOOL_QUERIES:
                (got,), st = run_bool(eng, [(terms, ms, k)])
                assert got == sm.bm.expected(terms, k, ms, rg), (rg, terms, ms, k)
                assert st.items == 1 and counters(st) == summed([sm.schedule(terms, ms, k, doc_range=rg)]), \
                    (rg, terms, ms, k)
        assert some > 0
    finally:
        eng.close()


# ---- the other entry points -----------------------------------------------------------------
def test_count_and_match_set_agree(stair):
    """wsr_count_bool never skips, so its answer is len(matching) whatever k
    says; wsr_docset_from_bool exports exactly the matching ids, those past
    65,535 included."""
    sm = stair.sm
    queries = BOOL_QUERIES + [(or_terms(t), 0) for t in ("lo mid hi", "lo lo hi", "lo lo2 mid hi")]
    want = [len(sm.stream(t, ms)) for t, ms in queries]
    for k in KS + (65, 0):
        got, st = run_count_ex(stair.eng, queries, k=k)
        assert got == want and st.windows_skipped == 0 and st.events == 0, k
    for name, ids in FILTERS.items():
        got, st = run_count(stair.eng, queries, [stair.sets[name]] * len(queries))
        assert got == [len(sm.stream(t, ms, None, ids)) for t, ms in queries] and st.windows_skipped == 0, name
    for (t, ms), n in zip(queries, want):
        with match_set(stair.eng, t, ms) as s:
            ids = s.ids().tolist()
            assert ids == [d for _, d in sm.stream(t, ms)] and s.count() == n and ids[-1] > 65535, (t, ms)
        with match_set(stair.eng, t, ms, within=stair.sets["hi_free"], item_blocks=1) as s:
            assert s.ids().tolist() == [d for _, d in sm.stream(t, ms, None, FILTERS["hi_free"])], (t, ms)
