"""GPU parity of the doc sets (wsr_docset, wiser_amd/csrc/docset.cc; kernels.hip
bool_filtered_kernel, count_filtered_kernel, match_set_kernel) against
tests/bool_model.py and heapmodel alone, with exact equality.  With F the
Python set of a filter's ids, the filtered stream is
    [(s, d) for s, d in bm.matching(terms, ms, doc_range) if d in F];
a search is rank_stream(stream, k)[0], a count its length, a match set its
docs.  The corpora are test_gpu_or.py's, the query sets test_gpu_bool.py's."""
import ctypes as C
import os
import subprocess
import threading

import pytest

from bool_model import BoolModel
from conftest import ROOT
from heapmodel import rank_stream
from test_gpu_bool import run_bool
from test_gpu_count import run_count as run_count_ex
from test_gpu_or import (EDGE_TERMS, _Ctx, _synth_queries, edge_ctx, skip_ctx, synth_ctx,  # noqa: F401
                         tie_ctx)

pytestmark = pytest.mark.gpu

M, S, N = "must", "should", "must_not"
N_DOCS = 20000   # the tie, skipping and synthetic corpora


def q(text, min_should=0):
    """'+a b -c' -> ([(a, must), (b, should), (c, must_not)], min_should)"""
    terms = []
    for t in text.split():
        terms.append((t[1:], M) if t[0] == "+" else (t[1:], N) if t[0] == "-" else (t, S))
    return terms, min_should


def _queries(eng, queries, ks):
    import wiser_amd as w
    from wiser_amd import _capi
    arr = (_capi.BoolQuery * len(queries))(*[eng.resolve_bool(w.BoolQuery(list(t), min_should=ms))[0]
                                             for t, ms in queries])
    for a, k in zip(arr, ks):
        a.k = k   # (the mirror clamps a negative k; the engine sees the caller's)
    return arr


def _filters(filters, n):
    """[DocSet or None] (or None: a NULL array) as the C ABI's array"""
    if filters is None:
        return None
    assert len(filters) == n
    return (C.c_void_p * n)(*[f._s if f is not None else None for f in filters])


def run_search(eng, queries, filters, item_blocks=0):
    """queries: [(terms, min_should, k)], filters: one DocSet or None each, in
    one wsr_search_bool_filtered call -> ([[(score, doc)]], wsr_or_stats)"""
    from wiser_amd import _capi
    n = len(queries)
    arr = _queries(eng, [(t, ms) for t, ms, _ in queries], [k for _, _, k in queries])
    stride = max(1, max(k for _, _, k in queries))
    hits, nh, st = (_capi.Hit * (n * stride))(), (C.c_int32 * n)(), _capi.OrStats()
    _capi.check(_capi.lib.wsr_search_bool_filtered(eng._h, arr, n, _filters(filters, n), stride, hits, nh,
                                                   item_blocks, C.byref(st)))
    got = [[(hits[i * stride + j].score, hits[i * stride + j].doc_id) for j in range(nh[i])] for i in range(n)]
    return got, st


def run_count(eng, queries, filters, item_blocks=0, k=10):
    """queries: [(terms, min_should)] in one wsr_count_bool_filtered call -> ([count], wsr_or_stats)"""
    from wiser_amd import _capi
    n = len(queries)
    arr = _queries(eng, queries, [k] * n)
    counts, st = (C.c_int64 * n)(*([-7] * n)), _capi.OrStats()
    _capi.check(_capi.lib.wsr_count_bool_filtered(eng._h, arr, n, _filters(filters, n), counts, item_blocks,
                                                  C.byref(st)))
    return list(counts), st


def plain_count(eng, queries):
    from wiser_amd import _capi
    n = len(queries)
    counts = (C.c_int64 * n)()
    _capi.check(_capi.lib.wsr_count_bool(eng._h, _queries(eng, queries, [10] * n), n, counts))
    return list(counts)


def match_set(eng, terms, ms, within=None, item_blocks=0):
    """wsr_docset_from_bool at an item length -> DocSet"""
    import wiser_amd as w
    from wiser_amd import _capi
    arr = _queries(eng, [(terms, ms)], [0])
    s = C.c_void_p()
    _capi.check(_capi.lib.wsr_docset_from_bool(eng._h, arr, within._s if within is not None else None, item_blocks,
                                               C.byref(s)))
    return w.DocSet(eng, s)


def stream(bm, terms, ms, ids, doc_range=None):
    """the model's filtered stream; ids: the filter's Python set, or None"""
    return [(s, d) for s, d in bm.matching(terms, ms, doc_range) if ids is None or d in ids]


_expected = {}   # (corpus, terms, ms, k, filter name) -> the model's answer, shared by the item lengths


def expected(key, make):
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


# ---- tie corpus ---------------------------------------------------------------
# (test_gpu_bool.py's TIE_QUERIES, restated)
MIX16 = ([("a", M), ("b", S), ("c", S), ("d", S), ("f3", N), ("b", S), ("c", S), ("a", M), ("d", S), ("zzz", S),
          ("c", S), ("b", S), ("zzz", N), ("d", S), ("f7", N), ("c", S)], 3)
TIE_QUERIES = ([q("+a +b"), q("+a b"), q("+a -b")] + [q("a b c d", ms) for ms in (1, 2, 3, 4, 5)] +
               [q("+d c -b"), q("-a b"), q("+a -a"), q("d d", 2), q("d d", 1), q("+zzz a"), q("a zzz", 2),
                q("-zzz +c"), MIX16])
TIE_KS = (1, 3, 10, 64, 65, 1024)
# name -> ids: every doc, none, every third doc, a range that begins and ends inside a window
FILTER_IDS = {"full": set(range(N_DOCS)), "empty": set(), "third": set(range(1, N_DOCS, 3)),
              "range": set(range(3000, 9500))}


@pytest.fixture(scope="module")
def tie_bm(tie_ctx):   # noqa: F811
    return BoolModel(tie_ctx.model)


@pytest.fixture(scope="module")
def tie_sets(tie_ctx):   # noqa: F811
    sets = {name: tie_ctx.eng.docset(sorted(ids)) for name, ids in FILTER_IDS.items()}
    yield sets
    for s in sets.values():
        s.close()


# ---- bitmap edges ------------------------------------------------------------------
def test_docset_bitmap_edges(tie_ctx):   # noqa: F811
    from wiser_amd import _capi
    eng = tie_ctx.eng
    assert eng.NumDocs() == N_DOCS
    cases = [[], [0], [N_DOCS - 1], [31, 32, 63, 64, 2047, 2048], [64, 5, 5, 19999, 0, 64, 2048, 5, 31],
             list(range(N_DOCS)), list(range(N_DOCS - 1, -1, -7))]
    for ids in cases:
        with eng.docset(ids) as s:
            assert s.count() == len(set(ids))
            got = s.ids()
            assert got.dtype.name == "int32" and got.tolist() == sorted(set(ids))
    # ids with cap too small: WSR_E_LIMIT, the number needed, nothing written
    with eng.docset([31, 32, 63, 64, 2047, 2048]) as s:
        for cap in (0, 5):
            out, n = (C.c_int32 * 8)(*([-7] * 8)), C.c_int64(-7)
            assert _capi.lib.wsr_docset_ids(eng._h, s._s, out, cap, C.byref(n)) == _capi.E_LIMIT
            assert n.value == 6 and list(out) == [-7] * 8
        out, n = (C.c_int32 * 8)(*([-7] * 8)), C.c_int64(-7)
        assert _capi.lib.wsr_docset_ids(eng._h, s._s, out, 6, C.byref(n)) == _capi.WSR_OK
        assert n.value == 6 and list(out) == [31, 32, 63, 64, 2047, 2048, -7, -7]
    # the empty set needs no room
    with eng.docset([]) as s:
        n = C.c_int64(-7)
        assert _capi.lib.wsr_docset_ids(eng._h, s._s, None, 0, C.byref(n)) == _capi.WSR_OK and n.value == 0


# ---- match sets -------------------------------------------------------------------------
@pytest.mark.parametrize("item_blocks", [63, 8, 1])
def test_match_sets_ties(tie_ctx, tie_bm, item_blocks):   # noqa: F811
    """ids equals the model's matching docs and count equals wsr_count_bool's
    answer; at one block per item two items share a bitmap word."""
    counts = plain_count(tie_ctx.eng, TIE_QUERIES)
    sizes = []
    for (t, ms), c in zip(TIE_QUERIES, counts):
        with match_set(tie_ctx.eng, t, ms, item_blocks=item_blocks) as s:
            want = [d for _, d in tie_bm.matching(t, ms)]
            assert s.ids().tolist() == want, (t, ms)
            assert s.count() == c == len(want), (t, ms)
            sizes.append(len(want))
    assert 0 in sizes and max(sizes) > 1024


@pytest.mark.parametrize("item_blocks", [63, 1])
def test_match_sets_edges(edge_ctx, item_blocks):   # noqa: F811
    bm = BoolModel(edge_ctx.model)
    sizes = []
    for a in EDGE_TERMS:
        for b in EDGE_TERMS:
            for ra, rb in ((M, S), (M, N), (S, N)):
                if a == b:
                    continue
                t = [(a, ra), (b, rb)]
                with match_set(edge_ctx.eng, t, 0, item_blocks=item_blocks) as s:
                    want = [d for _, d in bm.matching(t, 0)]
                    assert s.ids().tolist() == want and s.count() == len(want), t
                    sizes.append(len(want))
    assert min(sizes) == 0 < max(sizes)


@pytest.mark.parametrize("item_blocks", [63, 1])
def test_match_set_within(tie_ctx, tie_bm, tie_sets, item_blocks):   # noqa: F811
    """from_bool(q, within=S) is the model's set intersected with S, and sets compose."""
    for name in ("third", "range", "empty", "full"):
        for t, ms in TIE_QUERIES:
            with match_set(tie_ctx.eng, t, ms, within=tie_sets[name], item_blocks=item_blocks) as s:
                want = [d for _, d in stream(tie_bm, t, ms, FILTER_IDS[name])]
                assert s.ids().tolist() == want and s.count() == len(want), (name, t, ms)
    with match_set(tie_ctx.eng, *q("+c"), item_blocks=item_blocks) as c_set:
        with match_set(tie_ctx.eng, *q("+d"), within=c_set, item_blocks=item_blocks) as cd, \
                match_set(tie_ctx.eng, *q("a b", 2), within=cd, item_blocks=item_blocks) as abcd:
            want = [d for _, d in tie_bm.matching(*q("+a +b +c +d"))]
            assert abcd.ids().tolist() == want and len(want) > 0


# ---- filtered search ------------------------------------------------------------------------
def _complement_cases(bm):
    """Per (query, k): the complement of the query's own unfiltered top-k docs."""
    out = []
    for t, ms in TIE_QUERIES:
        for k in TIE_KS:
            top = {d for _, d in bm.expected(t, k, ms)}
            out.append((t, ms, k, set(range(N_DOCS)) - top))
    return out


def test_complement_filter_not_vacuous(tie_bm):
    """From the model alone: with the complement of the unfiltered top-k as the
    filter, the filtered top-k shares no doc with the unfiltered one although
    both are full, and equal scores lie on both sides of the filtered cut -- a
    filter applied after the threshold is built returns fewer or other docs."""
    differ = cut = 0
    for t, ms, k, ids in _complement_cases(tie_bm):
        plain = tie_bm.expected(t, k, ms)
        filt = rank_stream(stream(tie_bm, t, ms, ids), k)[0]
        if len(plain) == k and len(filt) == k:
            assert not {d for _, d in plain} & {d for _, d in filt}
            differ += 1
        sc = sorted((s for s, _ in stream(tie_bm, t, ms, ids)), reverse=True)
        cut += len(sc) > k and sc[k - 1] == sc[k]
    assert differ > 0 and cut > 0


@pytest.mark.parametrize("item_blocks", [63, 8, 1])
def test_filtered_search_ties(tie_ctx, tie_bm, tie_sets, item_blocks):   # noqa: F811
    eng = tie_ctx.eng
    qs = [(t, ms, k) for t, ms in TIE_QUERIES for k in TIE_KS]
    for name, ids in FILTER_IDS.items():
        got, st = run_search(eng, qs, [tie_sets[name]] * len(qs), item_blocks)
        bad = []
        for (t, ms, k), g in zip(qs, got):
            want = expected(("tie", str(t), ms, k, name), lambda: rank_stream(stream(tie_bm, t, ms, ids), k)[0])
            if g != want:
                bad.append((t, ms, k, g[:3], want[:3], len(g), len(want)))
        assert not bad, f"{name}: {len(bad)}/{len(qs)} differ (item_blocks={item_blocks}): {bad[:3]}"
        if name == "empty":
            assert not any(got) and st.windows == 0 and st.events == 0
        else:
            assert st.items > 0 and st.windows > 0 and st.events > 0
    # the complement of the query's own unfiltered top-k
    cases = _complement_cases(tie_bm)
    sets = [eng.docset(sorted(ids)) for _, _, _, ids in cases]
    try:
        got, _ = run_search(eng, [(t, ms, k) for t, ms, k, _ in cases], sets, item_blocks)
        bad = []
        for (t, ms, k, ids), g in zip(cases, got):
            want = expected(("tie", str(t), ms, k, "complement"),
                            lambda: rank_stream(stream(tie_bm, t, ms, ids), k)[0])
            if g != want:
                bad.append((t, ms, k, g[:3], want[:3], len(g), len(want)))
        assert not bad, f"complement: {len(bad)}/{len(cases)} differ (item_blocks={item_blocks}): {bad[:3]}"
    finally:
        for s in sets:
            s.close()


@pytest.mark.parametrize("item_blocks", [63, 1])
def test_filter_per_query(tie_ctx, tie_bm, tie_sets, item_blocks):   # noqa: F811
    """One call, a different filter per query, NULL entries included; a NULL
    array and all-NULL entries are the unfiltered call."""
    names = ["full", None, "third", "range", "empty", None]
    qs = [(t, ms, k) for t, ms in TIE_QUERIES for k in (3, 65)]
    which = [names[i % len(names)] for i in range(len(qs))]
    filters = [tie_sets[n] if n else None for n in which]
    got, _ = run_search(tie_ctx.eng, qs, filters, item_blocks)
    cnt, _ = run_count(tie_ctx.eng, [(t, ms) for t, ms, _ in qs], filters, item_blocks)
    for (t, ms, k), n, g, c in zip(qs, which, got, cnt):
        s = stream(tie_bm, t, ms, FILTER_IDS[n] if n else None)
        assert g == rank_stream(s, k)[0], (t, ms, k, n)
        assert c == len(s), (t, ms, n)
    for f in (None, [None] * len(qs)):
        got, _ = run_search(tie_ctx.eng, qs, f, item_blocks)
        assert got == [tie_bm.expected(t, k, ms) for t, ms, k in qs]
        cnt, _ = run_count(tie_ctx.eng, [(t, ms) for t, ms, _ in qs], f, item_blocks)
        assert cnt == [len(tie_bm.matching(t, ms)) for t, ms, _ in qs]


# ---- filtered count ---------------------------------------------------------------------------
@pytest.mark.parametrize("item_blocks", [63, 8, 1])
def test_filtered_count_ties(tie_ctx, tie_bm, tie_sets, item_blocks):   # noqa: F811
    eng = tie_ctx.eng
    for name, ids in FILTER_IDS.items():
        got, st = run_count(eng, TIE_QUERIES, [tie_sets[name]] * len(TIE_QUERIES), item_blocks)
        assert got == [len(stream(tie_bm, t, ms, ids)) for t, ms in TIE_QUERIES], name
        assert st.windows_skipped == 0 and st.events == 0
        assert (st.windows == 0) if name == "empty" else (max(got) > 0 and st.windows > 0)
    cases = _complement_cases(tie_bm)[2::6]   # (k = 10)
    sets = [eng.docset(sorted(ids)) for _, _, _, ids in cases]
    try:
        got, _ = run_count(eng, [(t, ms) for t, ms, _, _ in cases], sets, item_blocks)
        assert got == [len(stream(tie_bm, t, ms, ids)) for t, ms, _, ids in cases]
    finally:
        for s in sets:
            s.close()


def test_filtered_count_is_a_must_term(tie_ctx, tie_bm):   # noqa: F811
    """count(q, from_bool(+c)) == count(q with +c added), for queries that have a MUST term."""
    with_must = [(t, ms) for t, ms in TIE_QUERIES if any(r == M for _, r in t) and len(t) < 16]
    assert len(with_must) >= 5
    with match_set(tie_ctx.eng, *q("+c")) as c_set:
        got, _ = run_count(tie_ctx.eng, with_must, [c_set] * len(with_must))
    want = plain_count(tie_ctx.eng, [(t + [("c", M)], ms) for t, ms in with_must])
    assert got == want == [len(tie_bm.matching(t + [("c", M)], ms)) for t, ms in with_must]
    assert max(got) > 0


def test_filtered_count_ignores_k(tie_ctx, tie_bm, tie_sets):   # noqa: F811
    want = [len(stream(tie_bm, t, ms, FILTER_IDS["third"])) for t, ms in TIE_QUERIES]
    for k in (0, -5, 5000):
        got, _ = run_count(tie_ctx.eng, TIE_QUERIES, [tie_sets["third"]] * len(TIE_QUERIES), k=k)
        assert got == want, k


# ---- which windows run ----------------------------------------------------------------------------
def test_filtered_windows(skip_ctx):   # noqa: F811
    """A filter that is a doc range of two windows: only windows that overlap
    it run.  (`rare` is in docs 100.., 5000.., 10000.., 15000..; the range
    holds the third group.)"""
    eng = skip_ctx.eng
    bm = BoolModel(skip_ctx.model)
    lo, hi = 4 * 2048, 6 * 2048
    ids = set(range(lo, hi))
    with eng.docset(range(lo, hi)) as two, eng.docset([]) as none:
        for text, k in (("+rare common", 10), ("rare common", 10), ("+common -rare", 65)):
            t, ms = q(text)
            plain, pst = run_search(eng, [(t, ms, k)], None)
            got, st = run_search(eng, [(t, ms, k)], [two])
            assert got == [rank_stream(stream(bm, t, ms, ids), k)[0]] and got[0]
            assert 0 < st.windows <= 2 and st.windows < pst.windows, (text, st.windows, pst.windows)
            cnt, cst = run_count(eng, [(t, ms)], [two])
            assert cnt == [len(stream(bm, t, ms, ids))]
            assert 0 < cst.windows <= 2 and cst.windows_skipped == 0, (text, cst.windows)
            got, st = run_search(eng, [(t, ms, k)], [none])
            assert got == [[]] and st.windows == 0
            cnt, cst = run_count(eng, [(t, ms)], [none])
            assert cnt == [0] and cst.windows == 0 and cst.windows_skipped == 0
    # a set with one doc per second window: the windows between hold no doc of the set and do not run
    sparse = set(range(100, N_DOCS, 4096))
    with eng.docset(sorted(sparse)) as s:
        t, ms = q("+common rare")
        got, st = run_search(eng, [(t, ms, 10)], [s])
        assert got == [rank_stream(stream(bm, t, ms, sparse), 10)[0]] and len(got[0]) == len(sparse)
        assert 0 < st.windows <= len(sparse)
        cnt, cst = run_count(eng, [(t, ms)], [s])
        assert cnt == [len(sparse)] and 0 < cst.windows <= len(sparse)


# ---- identities on the synthetic index ----------------------------------------------------------------
def test_full_set_identities(synth_ctx):   # noqa: F811
    """With the full set the filtered kernels give the unfiltered calls'
    answers: hits, the five counters, counts."""
    from wiser_amd import _capi
    eng = synth_ctx.eng
    pairs = [t[:2] for t in _synth_queries(200, 77)]
    qs = [([(a, ra), (b, rb)], 0) for a, b in pairs for ra, rb in ((M, S), (M, N), (S, N))]
    n = len(qs)
    with eng.docset(range(eng.NumDocs())) as full:
        for k in (10, 100):
            arr = _queries(eng, qs, [k] * n)
            hits, nh, st = (_capi.Hit * (n * k))(), (C.c_int32 * n)(), _capi.OrStats()
            _capi.check(_capi.lib.wsr_search_bool_ex(eng._h, arr, n, k, hits, nh, 0, C.byref(st)))
            want = [[(hits[i * k + j].score, hits[i * k + j].doc_id) for j in range(nh[i])] for i in range(n)]
            got, fst = run_search(eng, [(t, ms, k) for t, ms in qs], [full] * n)
            assert got == want and sum(len(g) for g in got) > 0
            for f in ("items", "windows", "windows_skipped", "touched_docs", "events"):
                assert getattr(fst, f) == getattr(st, f), (k, f, getattr(fst, f), getattr(st, f))
            assert st.items > 0 and st.events > 0
        cnt, _ = run_count(eng, qs, [full] * n)
        assert cnt == plain_count(eng, qs) and max(cnt) > 0


# ---- doc-range shard engines -------------------------------------------------------------------------------
HAND4 = [(0, 128), (128, 7777), (7777, 7778), (7778, 20000)]


@pytest.mark.parametrize("cut", ["w3", "hand4"])
def test_filtered_shards(tie_ctx, tie_bm, cut):   # noqa: F811
    """A filter built from whole-index ids gives each shard the model
    restricted to its range, the counts sum to the whole, and a shard's
    from_bool sets no bit outside its range."""
    import wiser_amd as w
    ranges = HAND4 if cut == "hand4" else [(N_DOCS * r // 3, N_DOCS * (r + 1) // 3) for r in range(3)]
    ids = FILTER_IDS["third"]
    qs = [(t, ms, k) for t, ms in TIE_QUERIES for k in (10, 65)]
    total = [0] * len(TIE_QUERIES)
    for rg in ranges:
        eng = w.VacuumEngine(tie_ctx.eng.engine_dir_path, doc_range=rg, positions=False)
        eng.Load()
        try:
            with eng.docset(sorted(ids)) as s:
                assert s.count() == len(ids)   # (the set is over the whole index)
                for ib in (63, 1):
                    got, _ = run_search(eng, qs, [s] * len(qs), ib)
                    assert got == [rank_stream(stream(tie_bm, t, ms, ids, rg), k)[0] for t, ms, k in qs], (rg, ib)
                    cnt, _ = run_count(eng, TIE_QUERIES, [s] * len(TIE_QUERIES), ib)
                    assert cnt == [len(stream(tie_bm, t, ms, ids, rg)) for t, ms in TIE_QUERIES], (rg, ib)
                total = [a + b for a, b in zip(total, cnt)]
                for t, ms in TIE_QUERIES:
                    with match_set(eng, t, ms, item_blocks=1) as m, match_set(eng, t, ms, within=s) as mw:
                        assert m.ids().tolist() == [d for _, d in tie_bm.matching(t, ms, rg)]
                        assert mw.ids().tolist() == [d for _, d in stream(tie_bm, t, ms, ids, rg)]
        finally:
            eng.close()
    assert total == [len(stream(tie_bm, t, ms, ids)) for t, ms in TIE_QUERIES] and max(total) > 1024


# ---- limits ---------------------------------------------------------------------------------------------
def test_docset_errors(indexes):
    import wiser_amd as w
    from wiser_amd import _capi
    lib = _capi.lib
    eng, other = w.VacuumEngine(indexes["three"][0]), w.VacuumEngine(indexes["three"][0])
    eng.Load()
    other.Load()
    try:
        n_docs, n_lists = eng.NumDocs(), eng.TermCount()
        full, foreign = eng.docset(range(n_docs)), other.docset(range(n_docs))

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

        def search(arr, n, filters, stride=3, hits=True, nh=True, ib=0):
            h, c = (_capi.Hit * 6)(), (C.c_int32 * 2)(-7, -7)
            for e in h:
                e.doc_id = -7
            rc = lib.wsr_search_bool_filtered(eng._h, arr, n, filters, stride, h if hits else None,
                                              c if nh else None, ib, None)
            return rc, [e.doc_id for e in h] == [-7] * 6 and list(c) == [-7, -7]

        def count(arr, n, filters, out=True, ib=0):
            c = (C.c_int64 * 2)(-7, -7)
            rc = lib.wsr_count_bool_filtered(eng._h, arr, n, filters, c if out else None, ib, None)
            return rc, list(c) == [-7, -7]

        both = (C.c_void_p * 2)(full._s, full._s)
        # every wsr_search_bool / wsr_count_bool error through the filtered calls, outputs untouched
        cases = [(edit(n_terms=17), _capi.E_LIMIT), (edit(role1=3), _capi.E_INVALID),
                 (edit(min_should=-1), _capi.E_INVALID), (edit(n_terms=-1), _capi.E_INVALID),
                 (edit(list1=-2), _capi.E_INVALID), (edit(list1=n_lists), _capi.E_INVALID)]
        for b, code in cases:
            arr = (_capi.BoolQuery * 2)(base(), b)   # (the refused query second, after a good one)
            assert search(arr, 2, both) == (code, True), (code, lib.wsr_last_error())
            assert lib.wsr_last_error().startswith(b"query 1: ")
            assert count(arr, 2, both) == (code, True), (code, lib.wsr_last_error())
            assert lib.wsr_last_error().startswith(b"query 1: ")
        for b in (edit(k=_capi.MAX_K + 1), edit(k=4)):   # (k over WSR_MAX_K, k over the stride: search only)
            arr = (_capi.BoolQuery * 2)(base(), b)
            assert search(arr, 2, both) == (_capi.E_LIMIT, True)
        arr = (_capi.BoolQuery * 2)(base(), base())
        assert search(None, 2, both) == (_capi.E_INVALID, True)
        assert search(arr, 2, both, hits=False) == (_capi.E_INVALID, True)
        assert search(arr, 2, both, nh=False) == (_capi.E_INVALID, True)
        assert search(arr, -1, both) == (_capi.E_INVALID, True)
        assert search(arr, 2, both, ib=64) == (_capi.E_INVALID, True)
        assert count(None, 2, both) == (_capi.E_INVALID, True)
        assert count(arr, 2, both, out=False) == (_capi.E_INVALID, True)
        assert count(arr, -1, both) == (_capi.E_INVALID, True)
        assert count(arr, 2, both, ib=64) == (_capi.E_INVALID, True)
        # a set of another handle, anywhere
        mixed = (C.c_void_p * 2)(full._s, foreign._s)
        assert search(arr, 2, mixed) == (_capi.E_INVALID, True)
        assert lib.wsr_last_error().startswith(b"query 1: ") and b"another handle" in lib.wsr_last_error()
        assert count(arr, 2, mixed) == (_capi.E_INVALID, True)
        n, out, s = C.c_int64(-7), (C.c_int32 * 4)(-7, -7, -7, -7), C.c_void_p()
        assert lib.wsr_docset_count(eng._h, foreign._s, C.byref(n)) == _capi.E_INVALID and n.value == -7
        assert lib.wsr_docset_ids(eng._h, foreign._s, out, 4, C.byref(n)) == _capi.E_INVALID
        assert n.value == -7 and list(out) == [-7] * 4
        assert lib.wsr_docset_from_bool(eng._h, arr, foreign._s, 0, C.byref(s)) == _capi.E_INVALID and not s.value
        # ids outside [0, n_docs): no set is created
        for bad in (-1, n_docs):
            ids = (C.c_int32 * 3)(0, bad, 1)
            assert lib.wsr_docset_from_ids(eng._h, ids, 3, C.byref(s)) == _capi.E_INVALID and not s.value
            assert b"outside" in lib.wsr_last_error()
            with pytest.raises(_capi.WiserError) as e:
                eng.docset([0, bad])
            assert e.value.code == _capi.E_INVALID
        # from_bool: wsr_count_bool's checks; null arguments
        for b, code in cases:
            one = (_capi.BoolQuery * 1)(b)
            assert lib.wsr_docset_from_bool(eng._h, one, None, 0, C.byref(s)) == code and not s.value
        assert lib.wsr_docset_from_bool(eng._h, None, None, 0, C.byref(s)) == _capi.E_INVALID
        assert lib.wsr_docset_from_bool(eng._h, arr, None, 0, None) == _capi.E_INVALID
        assert lib.wsr_docset_from_bool(eng._h, arr, None, 64, C.byref(s)) == _capi.E_INVALID and not s.value
        assert lib.wsr_docset_from_ids(eng._h, None, 1, C.byref(s)) == _capi.E_INVALID and not s.value
        assert lib.wsr_docset_count(eng._h, None, C.byref(n)) == _capi.E_INVALID
        assert lib.wsr_docset_count(eng._h, full._s, None) == _capi.E_INVALID
        assert lib.wsr_docset_ids(eng._h, full._s, None, 4, C.byref(n)) == _capi.E_INVALID
        # nq = 0 is fine, with or without arrays
        assert search(None, 0, None, hits=False, nh=False) == (_capi.WSR_OK, True)
        assert search(arr, 0, both) == (_capi.WSR_OK, True)
        assert count(None, 0, None, out=False) == (_capi.WSR_OK, True)
        assert count(arr, 0, both) == (_capi.WSR_OK, True)
        assert eng.search_bool([], filters=[]) == [] and eng.count_bool([], filters=[]) == []
        # empty results, not errors: a query the host settles gives the empty set; k is ignored
        for text, ms in (("-hello -world", 0), ("+nosuchterm hello", 0), ("hello world", 3)):
            with eng.docset_from_bool(w.BoolQuery(q(text)[0], min_should=ms)) as e:
                assert e.count() == 0 and e.ids().tolist() == []
        with eng.docset_from_bool(w.BoolQuery([])) as e:
            assert e.count() == 0
        with eng.docset_from_bool(w.BoolQuery(q("hello")[0], n_results=0)) as e:
            assert e.count() == eng.lookup("hello")[1] > 0
        full.close()
        foreign.close()
    finally:
        eng.close()
        other.close()


# ---- concurrency and mirrors ----------------------------------------------------------------------------------
def test_two_threads_share_a_set(tie_ctx, tie_bm, tie_sets):   # noqa: F811
    ids, s = FILTER_IDS["third"], tie_sets["third"]
    qs = [(t, ms, 10) for t, ms in TIE_QUERIES]
    want = [rank_stream(stream(tie_bm, t, ms, ids), 10)[0] for t, ms, _ in qs]
    want_n = [len(stream(tie_bm, t, ms, ids)) for t, ms in TIE_QUERIES]
    errors = []

    def worker(ib):
        try:
            for _ in range(4):
                assert run_search(tie_ctx.eng, qs, [s] * len(qs), ib)[0] == want
                assert run_count(tie_ctx.eng, TIE_QUERIES, [s] * len(qs), ib)[0] == want_n
                with match_set(tie_ctx.eng, *q("+a b"), within=s, item_blocks=ib) as m:
                    assert m.count() == want_n[1]
        except BaseException as e:   # noqa: BLE001 - surfaced below
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(ib,)) for ib in (63, 8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
        assert not t.is_alive(), "a caller did not return"
    assert not errors, errors[:2]


@pytest.mark.parametrize("item_blocks", [0, 1])
def test_modes_share_contexts(tie_ctx, tie_bm, tie_sets, item_blocks):   # noqa: F811
    """One engine, one thread: every call takes the pooled context the call
    before it gave back, so a context sized by a count serves a larger search
    (its tables grow, its event and hit buffers are new to it), then a match
    set, filtered calls and a count again."""
    eng = tie_ctx.eng
    searches = [(t, ms, k) for t, ms in TIE_QUERIES for k in (3, 65, 1024)][:40]
    counted = (TIE_QUERIES * 3)[:40]

    def n_match(t, ms, name=None):
        return expected(("tie", str(t), ms, "count", name),
                        lambda: len(stream(tie_bm, t, ms, FILTER_IDS[name] if name else None)))

    def top(t, ms, k, name=None):
        return expected(("tie", str(t), ms, k, name),
                        lambda: rank_stream(stream(tie_bm, t, ms, FILTER_IDS[name] if name else None), k)[0])

    got, _ = run_count_ex(eng, counted[:3], item_blocks)
    assert got == [n_match(t, ms) for t, ms in counted[:3]]
    got, _ = run_bool(eng, searches, item_blocks)
    assert got == [top(t, ms, k) for t, ms, k in searches] and any(len(g) > 64 for g in got)
    with match_set(eng, *q("+a b"), item_blocks=item_blocks) as s:
        want = [d for _, d in tie_bm.matching(*q("+a b"))]
        assert s.ids().tolist() == want and s.count() == len(want) > 0
    names = ["third", None, "range", "empty", "full"]
    got, _ = run_count(eng, TIE_QUERIES[:5], [tie_sets[n] if n else None for n in names], item_blocks)
    assert got == [n_match(t, ms, n) for (t, ms), n in zip(TIE_QUERIES[:5], names)]
    two = [TIE_QUERIES[1] + (10,), TIE_QUERIES[4] + (65,)]
    got, _ = run_search(eng, two, [tie_sets["range"], tie_sets["third"]], item_blocks)
    assert got == [top(*two[0], "range"), top(*two[1], "third")] and all(got)
    got, _ = run_count_ex(eng, counted, item_blocks)
    assert got == [n_match(t, ms) for t, ms in counted] and max(got) > 1024


FIXTURE_QUERIES = {
    "three": [("*", q("+hello world")), ("i:0,2", q("hello +world -big")), ("i:1", q("wisconsin big")),
              ("i:", q("hello world")), ("b:+world", q("hello big")), ("b:hello,-big", q("hello world", 2)),
              ("i:2,0,2,1", q("+hello -nosuchterm")), ("b:+nosuchterm", q("hello"))],
    "order": [("i:4,0,2", q("+hello world")), ("b:+fill40,-fill45", q("again fill3", 2)), ("*", q("fill1 -fill30")),
              ("b:fill20,fill44", q("+again hello"))],
}


def _filter_ids(bm, n_docs, spec):
    if spec == "*":
        return None
    if spec.startswith("i:"):
        return {int(x) for x in spec[2:].split(",") if x}
    return {d for _, d in bm.matching(q(spec[2:].replace(",", " "))[0], 0)}


def _cli(index_dir, cases):
    """docset_cli's answer: [(count, [match set ids], [(score, doc)])]"""
    path = os.path.join(index_dir, "docset_queries.txt")
    with open(path, "w") as f:
        for spec, (t, ms) in cases:
            f.write(f"{spec} {ms} " + " ".join({M: "+", S: "", N: "-"}[r] + x for x, r in t) + "\n")
    out = subprocess.run([os.path.join(ROOT, "wiser_amd", "_lib", "docset_cli"), index_dir, path],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    res = []
    for line in out:
        c, ids, hits = [p.split() for p in line.split("|")]
        res.append((int(c[0]), [int(x) for x in ids],
                    [(float(h.split(":")[1]), int(h.split(":")[0])) for h in hits]))
    return res


def test_docset_fixtures(indexes):
    """Both mirrors and docset_cli on the suite's fixtures."""
    import wiser_amd as w
    for name, cases in FIXTURE_QUERIES.items():
        c = _Ctx(indexes[name][0])
        try:
            bm = BoolModel(c.model)
            n_docs = c.eng.NumDocs()
            want = []
            for spec, (t, ms) in cases:
                s = stream(bm, t, ms, _filter_ids(bm, n_docs, spec))
                want.append((len(s), [d for _, d in s], rank_stream(s, 10)[0]))
            assert any(n for n, _, _ in want)
            assert name != "three" or any(n == 0 for n, _, _ in want)
            sets = []
            for spec, _ in cases:
                if spec == "*":
                    sets.append(None)
                elif spec.startswith("i:"):
                    sets.append(c.eng.docset([int(x) for x in spec[2:].split(",") if x]))
                else:
                    sets.append(c.eng.docset_from_bool(w.BoolQuery(q(spec[2:].replace(",", " "))[0])))
            bqs = [w.BoolQuery(t, n_results=10, min_should=ms) for _, (t, ms) in cases]
            assert c.eng.count_bool(bqs, filters=sets) == [n for n, _, _ in want]
            res = c.eng.search_bool(bqs, filters=sets)
            assert [[(e.doc_score, e.doc_id) for e in r.entries] for r in res] == [h for _, _, h in want]
            for bq, s, (_, ids, _) in zip(bqs, sets, want):
                with c.eng.docset_from_bool(bq, within=s) as m:
                    assert m.ids().tolist() == ids and m.count() == len(ids)
            # calls without the keyword behave as before
            assert c.eng.count_bool(bqs) == [len(bm.matching(t, ms)) for _, (t, ms) in cases]
            assert _cli(indexes[name][0], cases) == want
            for s in sets:
                if s is not None:
                    s.close()
                    s.close()   # (closing twice is fine)
        finally:
            c.close()
