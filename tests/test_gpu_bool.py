"""GPU parity of the boolean queries (wsr_search_bool: bool_plan.cc,
kernels.hip bool_kernel, or_replay_kernel) against tests/bool_model.py: the
oracle's exact per-term contributions, the match rule, the left-to-right sum
and heapmodel.rank_stream.  Doc ids, order and f64 scores must be equal; there
is no tolerance.  The corpora are test_gpu_or.py's."""
import ctypes as C
import os
import random
import subprocess
import threading

import pytest

from bool_model import BoolModel
from conftest import ROOT, all_tokens
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


def run_bool(eng, queries, item_blocks=0):
    """queries: [(terms, min_should, k)] in one wsr_search_bool_ex call ->
    ([[(score, doc)]], wsr_or_stats)"""
    import wiser_amd as w
    from wiser_amd import _capi
    n = len(queries)
    arr = (_capi.BoolQuery * n)(*[eng.resolve_bool(w.BoolQuery(list(t), n_results=k, min_should=ms))[0]
                                  for t, ms, k in queries])
    for a, (_, _, k) in zip(arr, queries):
        a.k = k   # (the mirror clamps a negative k; the engine sees the caller's)
    stride = max(1, max(k for _, _, k in queries))
    hits, nh, st = (_capi.Hit * (n * stride))(), (C.c_int32 * n)(), _capi.OrStats()
    _capi.check(_capi.lib.wsr_search_bool_ex(eng._h, arr, n, stride, hits, nh, item_blocks, C.byref(st)))
    got = [[(hits[i * stride + j].score, hits[i * stride + j].doc_id) for j in range(nh[i])] for i in range(n)]
    return got, st


def check(ctx, bm, queries, item_blocks=0, eng=None, doc_range=None):
    got, st = run_bool(eng or ctx.eng, queries, item_blocks)
    bad = []
    for (t, ms, k), g in zip(queries, got):
        want = bm.expected(t, k, ms, doc_range)
        if g != want:
            bad.append((t, ms, k, g[:3], want[:3], len(g), len(want)))
    assert not bad, f"{len(bad)}/{len(queries)} boolean queries differ (item_blocks={item_blocks}): {bad[:3]}"
    return st


# ---- tie corpus ---------------------------------------------------------------
MIX16 = ([("a", M), ("b", S), ("c", S), ("d", S), ("f3", N), ("b", S), ("c", S), ("a", M), ("d", S), ("zzz", S),
          ("c", S), ("b", S), ("zzz", N), ("d", S), ("f7", N), ("c", S)], 3)
TIE_QUERIES = ([q("+a +b"), q("+a b"), q("+a -b")] + [q("a b c d", ms) for ms in (1, 2, 3, 4, 5)] +
               [q("+d c -b"), q("-a b"), q("+a -a"), q("d d", 2), q("d d", 1), q("+zzz a"), q("a zzz", 2),
                q("-zzz +c"), MIX16])
TIE_KS = (1, 3, 10, 64, 65, 1024)


@pytest.fixture(scope="module")
def tie_bm(tie_ctx):   # noqa: F811
    return BoolModel(tie_ctx.model)


def test_bool_tie_queries_not_vacuous(tie_bm):
    """From the model alone: the set loses docs to each rule, and some query
    has more matches than k with equal scores on both sides of the cut."""
    ex = [tie_bm.explain(t, ms) for t, ms in TIE_QUERIES]
    assert any(e.lost_not > 0 and e.matches > 0 for e in ex)
    assert any(e.lost_must > 0 and e.matches > 0 for e in ex)
    assert any(e.lost_should > 0 and e.matches > 0 for e in ex)
    assert len(MIX16[0]) == 16 and tie_bm.explain(*MIX16).matches > 0
    cut = 0
    for t, ms in TIE_QUERIES:
        sc = sorted((s for s, _ in tie_bm.matching(t, ms)), reverse=True)
        cut += sum(1 for k in TIE_KS if len(sc) > k and sc[k - 1] == sc[k])
    assert cut > 0
    for text, ms in (("a b c d", 5), ("+a -a", 0), ("+zzz a", 0), ("a zzz", 2)):
        assert tie_bm.matching(*q(text, ms)) == []
    assert tie_bm.matching(*q("d d", 2)) == tie_bm.matching(*q("d d", 1)) != []


@pytest.mark.parametrize("item_blocks", [63, 8, 1])
def test_bool_ties(tie_ctx, tie_bm, item_blocks):   # noqa: F811
    st = check(tie_ctx, tie_bm, [(t, ms, k) for t, ms in TIE_QUERIES for k in TIE_KS], item_blocks)
    assert st.items > 0 and st.windows > 0 and st.touched_docs >= st.events > 0


# ---- edge corpus ---------------------------------------------------------------
@pytest.mark.parametrize("item_blocks", [63, 1])
def test_bool_edges(edge_ctx, item_blocks):   # noqa: F811
    """Window edges, a VInts-only list and a single-posting list as lead, a
    lead whose postings skip whole windows."""
    bm = BoolModel(edge_ctx.model)
    qs = [([(a, ra), (b, rb)], 0, k) for a in EDGE_TERMS for b in EDGE_TERMS if a != b
          for ra, rb in ((M, S), (M, N), (S, N)) for k in (10, 200)]
    check(edge_ctx, bm, qs, item_blocks)


# ---- which lists start windows ---------------------------------------------------
def test_bool_windows(skip_ctx):   # noqa: F811
    bm = BoolModel(skip_ctx.model)
    st = check(skip_ctx, bm, [(*q("rare common"), 10)])
    assert st.windows_skipped > 0, (st.windows, st.windows_skipped)
    rare_windows = len({d // 2048 for d in skip_ctx.model.contrib("rare")})
    st = check(skip_ctx, bm, [(*q("+rare common"), 10)])
    assert 0 < st.windows <= rare_windows, (st.windows, rare_windows)
    st = check(skip_ctx, bm, [(*q("+common -rare"), 65)])
    assert len(bm.matching(*q("+common -rare"))) == 19960 == st.events and st.touched_docs == 20000


# ---- identities --------------------------------------------------------------------
def test_bool_identities(synth_ctx):   # noqa: F811
    """All MUST: the device's own conjunctive result; all SHOULD: match_any."""
    import wiser_amd as w
    qs = _synth_queries(200, 57)
    for role, any_ in ((M, False), (S, True)):
        for k in (10, 100):
            want = synth_ctx.eng.SearchBatch([w.SearchQuery(t, n_results=k, match_any=any_) for t in qs])
            got, _ = run_bool(synth_ctx.eng, [([(x, role) for x in t], 0, k) for t in qs])
            for t, g, r in zip(qs, got, want):
                assert g == [(e.doc_score, e.doc_id) for e in r.entries], (t, role, k)
            assert sum(len(g) for g in got) > 0


@pytest.mark.parametrize("item_blocks", [63, 1])
def test_bool_all_should_is_or(tie_ctx, skip_ctx, item_blocks):   # noqa: F811
    """bool_kernel and or_kernel are two instances of one traversal: an
    all-SHOULD wsr_search_bool_ex call and the same queries as WSR_QUERY_OR in
    one resident batch give equal hits and equal counters, all five."""
    for ctx, terms in ((tie_ctx, [["a", "b"], ["b", "a"], ["c", "d"], ["a", "b", "c", "d"]]),
                       (skip_ctx, [["common", "rare"], ["rare", "common"]])):
        qs = [(t, k) for t in terms for k in (10, 65)]
        want, ost = ctx.run(qs, item_blocks)
        got, bst = run_bool(ctx.eng, [([(x, S) for x in t], 0, k) for t, k in qs], item_blocks)
        assert got == want and all(want)
        for f in ("items", "windows", "windows_skipped", "touched_docs", "events"):
            assert getattr(bst, f) == getattr(ost, f), (f, getattr(bst, f), getattr(ost, f))
        assert ost.items > 0 and ost.events > 0


# ---- the suite's fixtures, through both mirrors ----------------------------------------
FIXTURE_QUERIES = {
    "three": [q("+hello world"), q("hello +world -big"), q("wisconsin big"), q("-hello world"), q("hello world", 2),
              q("+nosuchterm hello"), q("hello nosuchterm"), q("big big hello", 2), q("+hello -nosuchterm")],
    "order": [q("+hello world"), q("again fill3", 2), q("+fill40 -fill45 hello"), q("fill1 -fill30")],
}


def _cli(index_dir, queries, k):
    """bool_cli's answer: [([(score, doc)], doc_freqs)]"""
    path = os.path.join(index_dir, "bool_queries.txt")
    with open(path, "w") as f:
        for t, ms in queries:
            f.write(f"{ms} " + " ".join({M: "+", S: "", N: "-"}[r] + x for x, r in t) + "\n")
    out = subprocess.run([os.path.join(ROOT, "wiser_amd", "_lib", "bool_cli"), index_dir, path, str(k)],
                         check=True, capture_output=True, text=True).stdout.split("\n")
    res = []
    for i in range(len(queries)):
        ents = [(float.fromhex(e.split(":")[1]), int(e.split(":")[0])) for e in out[2 * i].split()]
        res.append((ents, [int(x) for x in out[2 * i + 1].split()]))
    return res


def test_bool_fixtures(indexes):
    import wiser_amd as w
    rng = random.Random(33)
    toks = all_tokens()
    tok_qs = []
    for _ in range(150):
        terms = [(t, rng.choice([M, S, S, N])) for t in rng.sample(toks, rng.choice([2, 3, 4]))]
        tok_qs.append((terms, rng.choice([0, 0, 1, 2])))
    for name, queries in (("three", FIXTURE_QUERIES["three"]), ("order", FIXTURE_QUERIES["order"]),
                          ("tok10k", tok_qs)):
        c = _Ctx(indexes[name][0])
        try:
            bm = BoolModel(c.model)
            for k in (1, 3, 10):
                res = c.eng.search_bool([w.BoolQuery(t, n_results=k, min_should=ms) for t, ms in queries])
                for (t, ms), r in zip(queries, res):
                    assert [(e.doc_score, e.doc_id) for e in r.entries] == bm.expected(t, k, ms), (name, t, ms, k)
                    assert r.doc_freqs == [c.orc.df(x) for x, _ in t]
            assert any(r.entries for r in res)
            # no terms / n_results 0: nothing, doc_freqs unset
            r0, r1 = c.eng.search_bool([w.BoolQuery([], n_results=3), w.BoolQuery(queries[0][0], n_results=0)])
            assert (r0.entries, r0.doc_freqs, r1.entries, r1.doc_freqs) == ([], [], [], [])
            for ((t, ms), (ents, dfs)) in zip(queries, _cli(indexes[name][0], queries, 3)):
                assert ents == bm.expected(t, 3, ms), (name, t, ms)
                assert dfs == [c.orc.df(x) for x, _ in t]
        finally:
            c.close()


# ---- doc-range shard engines ------------------------------------------------------------
HAND4 = [(0, 128), (128, 7777), (7777, 7778), (7778, 20000)]


@pytest.mark.parametrize("cut", ["w3", "hand4"])
def test_bool_shards(tie_ctx, tie_bm, cut):   # noqa: F811
    """Each shard's answer is the model restricted to the shard's docs (cuts
    inside blocks; hand4's third shard is doc 7777 alone)."""
    import wiser_amd as w
    n = 20000
    ranges = HAND4 if cut == "hand4" else [(n * r // 3, n * (r + 1) // 3) for r in range(3)]
    qs = [(t, ms, k) for t, ms in TIE_QUERIES for k in (10, 65)]
    some = 0
    for rg in ranges:
        eng = w.VacuumEngine(tie_ctx.eng.engine_dir_path, doc_range=rg, positions=False)
        eng.Load()
        try:
            for ib in (63, 1):
                check(tie_ctx, tie_bm, qs, ib, eng=eng, doc_range=rg)
            some += sum(1 for t, ms, k in qs if tie_bm.expected(t, k, ms, rg))
        finally:
            eng.close()
    assert some > 0


# ---- limits ---------------------------------------------------------------------------------
def test_bool_errors(indexes):
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

        cases = [(edit(n_terms=17), 4, _capi.E_LIMIT), (edit(k=_capi.MAX_K + 1), 2000, _capi.E_LIMIT),
                 (edit(k=4), 3, _capi.E_LIMIT), (edit(role1=3), 4, _capi.E_INVALID),
                 (edit(min_should=-1), 4, _capi.E_INVALID), (edit(n_terms=-1), 4, _capi.E_INVALID),
                 (edit(list1=-2), 4, _capi.E_INVALID), (edit(list1=n_lists), 4, _capi.E_INVALID)]
        for b, stride, code in cases:
            hits, nh = (_capi.Hit * 4)(), (C.c_int32 * 2)(-7, -7)
            for j in range(4):
                hits[j].doc_id, hits[j].score = -7, -7.0
            # (the refused query second, after a good one: nothing of the call may be written)
            arr = (_capi.BoolQuery * 2)(base(), b)
            assert lib.wsr_search_bool(eng._h, arr, 2, stride, hits, nh) == code, (code, lib.wsr_last_error())
            assert lib.wsr_last_error().startswith(b"query 1: ")
            assert list(nh) == [-7, -7] and all(h.doc_id == -7 and h.score == -7.0 for h in hits)
            if stride == 4:   # (the per-query checks alone know nothing of a hit stride)
                assert lib.wsr_check_bool_query(eng._h, C.byref(b)) == code
        assert lib.wsr_check_bool_query(eng._h, C.byref(base())) == _capi.WSR_OK
        assert lib.wsr_check_bool_query(eng._h, C.byref(edit(k=4))) == _capi.WSR_OK
        # null arguments with nq > 0; a negative nq
        one, hits, nh = (_capi.BoolQuery * 1)(base()), (_capi.Hit * 4)(), (C.c_int32 * 1)(-7)
        assert lib.wsr_search_bool(eng._h, None, 1, 4, hits, nh) == _capi.E_INVALID
        assert lib.wsr_search_bool(eng._h, one, 1, 4, None, nh) == _capi.E_INVALID
        assert lib.wsr_search_bool(eng._h, one, 1, 4, hits, None) == _capi.E_INVALID
        assert lib.wsr_search_bool(None, one, 1, 4, hits, nh) == _capi.E_INVALID
        assert lib.wsr_search_bool(eng._h, one, -1, 4, hits, nh) == _capi.E_INVALID
        assert nh[0] == -7
        # nq = 0 is fine, with or without arrays
        assert lib.wsr_search_bool(eng._h, None, 0, 0, None, None) == _capi.WSR_OK
        assert lib.wsr_search_bool(eng._h, one, 0, 4, hits, nh) == _capi.WSR_OK and nh[0] == -7
        assert eng.search_bool([]) == []
        # empty results are not errors: k <= 0 (any stride), no terms, MUST_NOT only, min_should out of reach
        for b in (edit(k=0), edit(k=-3), edit(n_terms=0), edit(min_should=2)):
            one[0], nh[0] = b, -7
            assert lib.wsr_search_bool(eng._h, one, 1, 4, hits, nh) == _capi.WSR_OK and nh[0] == 0
        nots = eng.resolve_bool(w.BoolQuery(q("-hello -world")[0], n_results=3))[0]
        one[0], nh[0] = nots, -7
        assert lib.wsr_search_bool(eng._h, one, 1, 4, hits, nh) == _capi.WSR_OK and nh[0] == 0
        with pytest.raises(_capi.WiserError) as e:
            eng.search_bool([w.BoolQuery([("hello", S)] * 17)])
        assert e.value.code == _capi.E_LIMIT
        assert eng.search_bool([w.BoolQuery([("hello", S)] * 16, n_results=3)])[0].Size() == 3
    finally:
        eng.close()


def test_bool_two_threads(tie_ctx, tie_bm):   # noqa: F811
    """Concurrent calls on one handle: each works in a context of its own."""
    qs = [(t, ms, k) for t, ms in TIE_QUERIES for k in (10, 65)]
    want = [tie_bm.expected(t, k, ms) for t, ms, k in qs]
    errors = []

    def worker(ib):
        try:
            for _ in range(4):
                got, _ = run_bool(tie_ctx.eng, qs, ib)
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
