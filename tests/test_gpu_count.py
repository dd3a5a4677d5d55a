"""GPU parity of the exact match counts (wsr_count_bool: bool_plan.cc
plan_count, kernels.hip count_kernel) against tests/bool_model.py alone:
len(BoolModel.matching(terms, min_should, doc_range)), with exact equality.
The corpora are test_gpu_or.py's, the query sets test_gpu_bool.py's."""
import ctypes as C
import os
import subprocess
import threading

import pytest

from bool_model import BoolModel
from conftest import ROOT
from test_gpu_or import (EDGE_TERMS, _Ctx, _synth_queries, edge_ctx, skip_ctx, synth_ctx,  # noqa: F401
                         tie_ctx)

pytestmark = pytest.mark.gpu

M, S, N = "must", "should", "must_not"


def q(text, min_should=0):
    """'+a b -c' -> ([(a, must), (b, should), (c, must_not)], min_should)"""
    terms = []
    for t in text.split():
        terms.append((t[1:], M) if t[0] == "+" else (t[1:], N) if t[0] == "-" else (t, S))
    return terms, min_should


def run_count(eng, queries, item_blocks=0, k=10):
    """queries: [(terms, min_should)] in one wsr_count_bool_ex call, every
    query's k set to `k` -> ([count], wsr_or_stats)"""
    import wiser_amd as w
    from wiser_amd import _capi
    n = len(queries)
    arr = (_capi.BoolQuery * n)(*[eng.resolve_bool(w.BoolQuery(list(t), min_should=ms))[0] for t, ms in queries])
    for a in arr:
        a.k = k
    counts, st = (C.c_int64 * n)(*([-7] * n)), _capi.OrStats()
    _capi.check(_capi.lib.wsr_count_bool_ex(eng._h, arr, n, counts, item_blocks, C.byref(st)))
    return list(counts), st


def check(bm, eng, queries, item_blocks=0, doc_range=None, k=10):
    got, st = run_count(eng, queries, item_blocks, k)
    want = [len(bm.matching(t, ms, doc_range)) for t, ms in queries]
    bad = [(t, ms, g, w_) for (t, ms), g, w_ in zip(queries, got, want) if g != w_]
    assert not bad, f"{len(bad)}/{len(queries)} counts differ (item_blocks={item_blocks}): {bad[:3]}"
    assert st.events == 0 and st.windows_skipped == 0
    return got, st


# ---- tie corpus ---------------------------------------------------------------
# (test_gpu_bool.py's TIE_QUERIES, restated)
MIX16 = ([("a", M), ("b", S), ("c", S), ("d", S), ("f3", N), ("b", S), ("c", S), ("a", M), ("d", S), ("zzz", S),
          ("c", S), ("b", S), ("zzz", N), ("d", S), ("f7", N), ("c", S)], 3)
TIE_QUERIES = ([q("+a +b"), q("+a b"), q("+a -b")] + [q("a b c d", ms) for ms in (1, 2, 3, 4, 5)] +
               [q("+d c -b"), q("-a b"), q("+a -a"), q("d d", 2), q("d d", 1), q("+zzz a"), q("a zzz", 2),
                q("-zzz +c"), MIX16])


@pytest.fixture(scope="module")
def tie_bm(tie_ctx):   # noqa: F811
    return BoolModel(tie_ctx.model)


def test_count_tie_queries_not_vacuous(tie_bm):
    """From the model alone: the set holds a count of 0, a count above 1,024,
    queries that lose docs to each of the three rules, and a min_should >= 2
    query whose count differs from its min_should = 1 count."""
    n = [len(tie_bm.matching(t, ms)) for t, ms in TIE_QUERIES]
    assert 0 in n and max(n) > 1024
    ex = [tie_bm.explain(t, ms) for t, ms in TIE_QUERIES]
    assert any(e.lost_must > 0 and e.matches > 0 for e in ex)
    assert any(e.lost_not > 0 and e.matches > 0 for e in ex)
    assert any(e.lost_should > 0 and e.matches > 0 for e in ex)
    abcd = {ms: len(tie_bm.matching(*q("a b c d", ms))) for ms in (1, 2, 3, 4, 5)}
    assert abcd[1] > abcd[2] > abcd[3] > abcd[4] > abcd[5] == 0
    assert len(MIX16[0]) == 16 and MIX16[1] >= 2 and tie_bm.explain(*MIX16).matches > 0


@pytest.mark.parametrize("item_blocks", [63, 8, 1])
def test_count_ties(tie_ctx, tie_bm, item_blocks):   # noqa: F811
    got, st = check(tie_bm, tie_ctx.eng, TIE_QUERIES, item_blocks)
    assert st.items > 0 and st.windows > 0 and st.touched_docs >= max(got) > 1024


# ---- edge corpus ---------------------------------------------------------------
@pytest.mark.parametrize("item_blocks", [63, 1])
def test_count_edges(edge_ctx, item_blocks):   # noqa: F811
    """Window edges, a VInts-only list and a single-posting list as lead, a
    lead whose postings skip whole windows."""
    bm = BoolModel(edge_ctx.model)
    qs = [([(a, ra), (b, rb)], 0) for a in EDGE_TERMS for b in EDGE_TERMS if a != b
          for ra, rb in ((M, S), (M, N), (S, N))]
    got, _ = check(bm, edge_ctx.eng, qs, item_blocks)
    assert min(got) == 0 < max(got)


# ---- which lists start windows ---------------------------------------------------
def test_count_windows(skip_ctx):   # noqa: F811
    bm = BoolModel(skip_ctx.model)
    rare_windows = len({d // 2048 for d in skip_ctx.model.contrib("rare")})
    got, st = check(bm, skip_ctx.eng, [q("+rare common")])
    assert got == [40] and 0 < st.windows <= rare_windows, (st.windows, rare_windows)
    got, st = check(bm, skip_ctx.eng, [q("+common -rare")])
    assert got == [19960] and st.touched_docs == 20000
    # MUST_NOT slots start no window; without a MUST term every SHOULD slot does
    got, st = check(bm, skip_ctx.eng, [q("rare -common")])
    assert got == [0] and 0 < st.windows <= rare_windows
    got, st = check(bm, skip_ctx.eng, [q("rare common")])
    assert got == [20000] == [st.touched_docs]


# ---- identities on the device ------------------------------------------------------
def _nhits(eng, queries, k):
    """wsr_search_bool's n_hits of [(terms, min_should)] at k"""
    import wiser_amd as w
    from wiser_amd import _capi
    n = len(queries)
    arr = (_capi.BoolQuery * n)(*[eng.resolve_bool(w.BoolQuery(list(t), n_results=k, min_should=ms))[0]
                                  for t, ms in queries])
    hits, nh = (_capi.Hit * (n * k))(), (C.c_int32 * n)()
    _capi.check(_capi.lib.wsr_search_bool(eng._h, arr, n, k, hits, nh))
    return list(nh)


def test_count_identities(synth_ctx):   # noqa: F811
    eng = synth_ctx.eng
    pairs = [(t[0], t[1]) for t in _synth_queries(200, 91)]
    df = {x: eng.lookup(x)[1] for p in pairs for x in p}
    singles = sorted(df)
    for role in (M, S):
        got, _ = run_count(eng, [([(x, role)], 0) for x in singles])
        assert got == [df[x] for x in singles]
    assert max(df.values()) > 0
    both, _ = run_count(eng, [([(a, M), (b, M)], 0) for a, b in pairs])
    either, _ = run_count(eng, [([(a, S), (b, S)], 0) for a, b in pairs])
    a_not_b, _ = run_count(eng, [([(a, M), (b, N)], 0) for a, b in pairs])
    for (a, b), n_and, n_or, n_not in zip(pairs, both, either, a_not_b):
        assert n_or == df[a] + df[b] - n_and, (a, b)
        assert df[a] == n_and + n_not, (a, b)
    assert sum(both) > 0
    # against wsr_search_bool's n_hits at k = 1,024, on the whole queries in three role forms
    qs = []
    for i, t in enumerate(_synth_queries(200, 92)):
        roles = [(M,) * len(t), (S,) * len(t), (M,) + (S,) * (len(t) - 2) + (N,)][i % 3]
        qs.append((list(zip(t, roles)), 0))
    got, _ = run_count(eng, qs)
    nh = _nhits(eng, qs, 1024)
    below = above = 0
    for (t, _), c, h in zip(qs, got, nh):
        assert c >= h, (t, c, h)
        if c <= 1024:
            assert c == h, (t, c, h)
            below += c > 0
        else:
            assert h == 1024, (t, c, h)
            above += 1
    assert below > 0 and above > 0, (below, above)


def test_count_ignores_k(tie_ctx, tie_bm):   # noqa: F811
    for k in (0, -5, 10, 5000):
        check(tie_bm, tie_ctx.eng, TIE_QUERIES, k=k)


# ---- doc-range shard engines ------------------------------------------------------------
HAND4 = [(0, 128), (128, 7777), (7777, 7778), (7778, 20000)]


@pytest.mark.parametrize("cut", ["w3", "hand4"])
def test_count_shards(tie_ctx, tie_bm, cut):   # noqa: F811
    """Each shard counts the model restricted to its docs (cuts inside
    blocks; hand4's third shard is doc 7777 alone) and the shards of the
    partition add up to the whole-index count."""
    import wiser_amd as w
    n = 20000
    ranges = HAND4 if cut == "hand4" else [(n * r // 3, n * (r + 1) // 3) for r in range(3)]
    whole, _ = check(tie_bm, tie_ctx.eng, TIE_QUERIES)
    total = [0] * len(TIE_QUERIES)
    for rg in ranges:
        eng = w.VacuumEngine(tie_ctx.eng.engine_dir_path, doc_range=rg, positions=False)
        eng.Load()
        try:
            for ib in (63, 1):
                got, _ = check(tie_bm, eng, TIE_QUERIES, ib, doc_range=rg)
            total = [a + b for a, b in zip(total, got)]
        finally:
            eng.close()
    assert total == whole and max(whole) > 1024


# ---- limits ---------------------------------------------------------------------------------
def test_count_errors(indexes):
    import wiser_amd as w
    from wiser_amd import _capi
    lib = _capi.lib
    eng = w.VacuumEngine(indexes["three"][0])
    eng.Load()
    try:
        n_lists = eng.TermCount()

        def base():
            return eng.resolve_bool(w.BoolQuery(q("+hello world")[0], n_results=3))[0]

        def edit(**kw):
            b = base()
            for name, v in kw.items():
                if name in ("list1", "role1"):
                    (b.list_ids if name == "list1" else b.role)[1] = v
                else:
                    setattr(b, name, v)
            return b

        cases = [(edit(n_terms=17), _capi.E_LIMIT), (edit(role1=3), _capi.E_INVALID),
                 (edit(min_should=-1), _capi.E_INVALID), (edit(n_terms=-1), _capi.E_INVALID),
                 (edit(list1=-2), _capi.E_INVALID), (edit(list1=n_lists), _capi.E_INVALID)]
        for b, code in cases:
            # (the refused query second, after a good one: nothing of the call may be written)
            arr, counts = (_capi.BoolQuery * 2)(base(), b), (C.c_int64 * 2)(-7, -7)
            assert lib.wsr_count_bool(eng._h, arr, 2, counts) == code, (code, lib.wsr_last_error())
            assert lib.wsr_last_error().startswith(b"query 1: ")
            assert list(counts) == [-7, -7]
        # null arguments with nq > 0; a negative nq; item blocks out of range
        one, counts = (_capi.BoolQuery * 1)(base()), (C.c_int64 * 1)(-7)
        assert lib.wsr_count_bool(eng._h, None, 1, counts) == _capi.E_INVALID
        assert lib.wsr_count_bool(eng._h, one, 1, None) == _capi.E_INVALID
        assert lib.wsr_count_bool(None, one, 1, counts) == _capi.E_INVALID
        assert lib.wsr_count_bool(eng._h, one, -1, counts) == _capi.E_INVALID
        assert lib.wsr_count_bool_ex(eng._h, one, 1, counts, 64, None) == _capi.E_INVALID
        assert counts[0] == -7
        # nq = 0 is fine, with or without arrays
        assert lib.wsr_count_bool(eng._h, None, 0, None) == _capi.WSR_OK
        assert lib.wsr_count_bool(eng._h, one, 0, counts) == _capi.WSR_OK and counts[0] == -7
        assert eng.count_bool([]) == []
        # a count of 0 is a result: no terms, min_should out of reach, MUST_NOT only, a missing MUST term;
        # the stats of a call that never reached the device are all 0
        nots = eng.resolve_bool(w.BoolQuery(q("-hello -world")[0]))[0]
        gone = eng.resolve_bool(w.BoolQuery(q("+nosuchterm hello")[0]))[0]
        for b in (edit(n_terms=0), edit(min_should=2), nots, gone):
            one[0], counts[0] = b, -7
            st = _capi.OrStats(9, 9, 9, 9, 9)
            assert lib.wsr_count_bool_ex(eng._h, one, 1, counts, 0, C.byref(st)) == _capi.WSR_OK and counts[0] == 0
            assert (st.items, st.windows, st.windows_skipped, st.touched_docs, st.events) == (0, 0, 0, 0, 0)
        # k is no error and no empty result
        for k in (0, -3, _capi.MAX_K + 1):
            one[0], counts[0] = edit(k=k), -7
            assert lib.wsr_count_bool(eng._h, one, 1, counts) == _capi.WSR_OK and counts[0] > 0
        with pytest.raises(_capi.WiserError) as e:
            eng.count_bool([w.BoolQuery([("hello", S)] * 17)])
        assert e.value.code == _capi.E_LIMIT
        assert eng.count_bool([w.BoolQuery([("hello", S)] * 16)]) == [eng.lookup("hello")[1]]
    finally:
        eng.close()


def test_count_two_threads(tie_ctx, tie_bm):   # noqa: F811
    """Concurrent calls on one handle: each works in a context of its own."""
    want = [len(tie_bm.matching(t, ms)) for t, ms in TIE_QUERIES]
    errors = []

    def worker(ib):
        try:
            for _ in range(4):
                got, _ = run_count(tie_ctx.eng, TIE_QUERIES, ib)
                assert got == want
        except BaseException as e:   # noqa: BLE001 - surfaced below
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(ib,)) for ib in (63, 8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
        assert not t.is_alive(), "a caller did not return"
    assert not errors, errors[:2]


# ---- the suite's fixtures, through both mirrors ----------------------------------------
FIXTURE_QUERIES = {
    "three": [q("+hello world"), q("hello +world -big"), q("wisconsin big"), q("-hello world"), q("hello world", 2),
              q("+nosuchterm hello"), q("hello nosuchterm"), q("big big hello", 2), q("+hello -nosuchterm")],
    "order": [q("+hello world"), q("again fill3", 2), q("+fill40 -fill45 hello"), q("fill1 -fill30")],
}


def _cli(index_dir, queries):
    """count_cli's answer: [count]"""
    path = os.path.join(index_dir, "count_queries.txt")
    with open(path, "w") as f:
        for t, ms in queries:
            f.write(f"{ms} " + " ".join({M: "+", S: "", N: "-"}[r] + x for x, r in t) + "\n")
    out = subprocess.run([os.path.join(ROOT, "wiser_amd", "_lib", "count_cli"), index_dir, path],
                         check=True, capture_output=True, text=True).stdout.split()
    return [int(x) for x in out]


def test_count_fixtures(indexes):
    import wiser_amd as w
    from wiser_amd import _capi
    for name, queries in FIXTURE_QUERIES.items():
        c = _Ctx(indexes[name][0])
        try:
            bm = BoolModel(c.model)
            want = [len(bm.matching(t, ms)) for t, ms in queries]
            assert any(want)
            assert c.eng.count_bool([w.BoolQuery(t, min_should=ms) for t, ms in queries]) == want
            assert c.eng.count_bool([w.BoolQuery(t, n_results=0, min_should=ms) for t, ms in queries]) == want
            assert _cli(indexes[name][0], queries) == want
            # count(SearchQuery): all MUST, or all SHOULD with match_any
            for terms in (["hello", "world"], ["hello"], ["hello", "nosuchterm"], []):
                for any_, role in ((False, M), (True, S)):
                    n = c.eng.count(w.SearchQuery(terms, match_any=any_))
                    assert n == len(bm.matching([(x, role) for x in terms])), (name, terms, any_)
            assert c.eng.count(w.SearchQuery(["hello", "world"], match_any=True)) > 0
            with pytest.raises(_capi.WiserError) as e:
                c.eng.count(w.SearchQuery(["hello", "world"], is_phrase=True))
            assert e.value.code == _capi.E_INVALID
            with pytest.raises(_capi.WiserError) as e:
                c.eng.count(w.SearchQuery(["hello"] * 17))
            assert e.value.code == _capi.E_LIMIT
        finally:
            c.close()
