"""GPU parity of wsr_score_docs (kernels.hip score_docs_kernel: what a query
gives each of the caller's docs) against the oracle alone: or_model's exact
per-term contributions, summed per doc from 0.0 in query order over the terms
whose lists hold the doc; the mask from membership.  Scores and masks must be
equal; there is no tolerance.

Every corpus test asserts that its pairs include full, partial and zero masks,
so that none passes on hits or on misses alone."""
import ctypes as C
import os
import random
import subprocess
import threading

import pytest

from conftest import ROOT, all_tokens
from or_model import OrModel
from test_gpu_or import TIE_QUERIES, _Ctx, tie_ctx  # noqa: F401  (tie_ctx: the tie corpus' fixture)
from test_gpu_parity import DENSE_MODES, _engine

pytestmark = pytest.mark.gpu


def expected(model, terms, docs):
    """-> [(score, mask)] of docs for the query `terms`, from the oracle"""
    contribs = [model.contrib(t) for t in terms]
    out = []
    for d in docs:
        s, m = 0.0, 0
        for t, c in enumerate(contribs):
            if c and d in c:
                s = s + c[d]
                m |= 1 << t
        out.append((s, m))
    return out


def kinds(terms, rows):
    """which of full / partial / zero masks the rows of one query show"""
    full = (1 << len(terms)) - 1
    return {"zero" if m == 0 else "full" if m == full else "partial" for _, m in rows}


def check(eng, model, cases):
    """cases: [(terms, docs)] in one call; -> the kinds of masks seen"""
    import wiser_amd as w
    got = eng.score_docs_batch([w.SearchQuery(list(t)) for t, _ in cases], [d for _, d in cases])
    seen = set()
    for (t, d), g in zip(cases, got):
        want = expected(model, t, d)
        bad = [(x, a, b) for x, a, b in zip(d, g, want) if a != b]
        assert not bad and len(g) == len(d), (t, len(bad), bad[:3])
        seen |= kinds(t, want)
    return seen


def postings(model, t):
    return sorted(model.contrib(t))


ALL_KINDS = {"full", "partial", "zero"}


# ---- 1. fixtures of the suite ----------------------------------------------
@pytest.mark.parametrize("name", ["three", "order", "tok10k"])
def test_score_docs_fixtures(indexes, name):
    rng = random.Random(33)
    if name == "three":
        queries = [["hello", "world"], ["world", "hello"], ["wisconsin", "big"], ["hello"], ["nosuchterm", "world"],
                   ["big", "big", "hello"], ["wisconsin", "big", "world"]]
    elif name == "order":
        queries = [["hello", "world"], ["again", "fill3"], ["fill40", "hello"], ["fill1"], ["fill45", "fill30", "fill12"]]
    else:
        toks = all_tokens()
        queries = [rng.sample(toks, n) for n in (1, 2, 3) for _ in range(12)]
    c = _Ctx(indexes[name][0])
    try:
        n = c.eng.NumDocs()
        cases = []
        for q in queries:
            docs = sorted({d for t in q for d in (c.model.contrib(t) or {})})   # every doc of the OR result
            docs += [rng.randrange(n) for _ in range(50)] + [0, n - 1]
            cases.append((q, docs))
        assert check(c.eng, c.model, cases) == ALL_KINDS
        # the single-query form
        q, docs = cases[0]
        import wiser_amd as w
        assert c.eng.score_docs(w.SearchQuery(q), docs) == expected(c.model, q, docs)
    finally:
        c.close()


# ---- 2. the tie corpus: the kernel's edges ----------------------------------
QUERIES = TIE_QUERIES + [["d", "zzz", "c", "a"] * 4]
N_TIE = 20000


def tie_candidate_sets(model):
    """name -> doc ids, chosen from the block structure of the lists (128
    postings per block, a VInts block for the rest)"""
    rng = random.Random(9)
    a, c, d = (postings(model, t) for t in "acd")
    assert len(a) == N_TIE and len(a) // 128 == 156 and len(c) // 128 >= 64 and len(c) % 128 and len(d) % 128
    sets = {}
    sets["block_first_last"] = [p[128 * j + o] for p in (c, d) for j in (0, 1, 17, len(p) // 128 - 1) for o in (0, 127)]
    gaps = [x for p in (c, d) for j in range(1, len(p) // 128) for x in range(p[128 * j - 1] + 1, p[128 * j])]
    assert len(gaps) > 20   # docs between the last posting of a block and the first of the next
    sets["block_gaps"] = gaps[:40]
    below = [x for p in (c, d) for x in range(p[0])]
    above = [x for p in (c, d) for x in range(p[-1] + 1, N_TIE)]
    assert below and above
    sets["below_first_above_last"] = below[:5] + above[-5:]
    sets["vints_tail"] = [x for p in (c, d) for x in (p[len(p) // 128 * 128], p[-1], p[-1] - 1, p[-2])]
    sets["tf300"] = [7777, 7776, 7778]
    sets["one_block_64"] = c[128 * 3 + 10:128 * 3 + 74]
    sets["blocks_64"] = [c[128 * j + 5 + j % 3] for j in range(64)]
    sets["exactly_64"] = rng.sample(range(N_TIE), 64)
    sets["exactly_65"] = rng.sample(range(N_TIE), 65)
    sets["exactly_1"] = [d[200]]
    sets["none"] = []
    sets["duplicates"] = [c[300]] * 3 + [5, 5, d[128], c[300], 7777, 7777] + [a[4000]] * 70
    sets["reversed"] = list(range(9000, 8800, -1))
    sets["shuffled"] = rng.sample(range(N_TIE), 300)
    sets["cuts_of_three_shards"] = [6665, 6666, 6667, 13332, 13333, 13334, 0, N_TIE - 1]
    assert [len(sets[k]) for k in ("one_block_64", "blocks_64", "exactly_64", "exactly_65")] == [64, 64, 64, 65]
    return sets


@pytest.fixture(scope="module")
def tie_cases(tie_ctx):  # noqa: F811
    """every candidate set under every query, in the order of the sets (the
    empty set between two that have some), and what the oracle says of them"""
    sets = tie_candidate_sets(tie_ctx.model)
    cases = [(q, docs) for q in QUERIES for docs in sets.values()]
    return cases, [expected(tie_ctx.model, q, d) for q, d in cases]


def test_score_docs_ties(tie_ctx, tie_cases):  # noqa: F811
    import wiser_amd as w
    cases, want = tie_cases
    assert any(not d for _, d in cases[1:-1])
    got = tie_ctx.eng.score_docs_batch([w.SearchQuery(q) for q, _ in cases], [d for _, d in cases])
    for (q, d), g, x in zip(cases, got, want):
        assert g == x, (q, d[:5], [(i, a, b) for i, a, b in zip(d, g, x) if a != b][:3])
    # the three kinds of masks, for ["c", "d"] alone too
    assert set().union(*[kinds(q, x) for (q, _), x in zip(cases, want)]) == ALL_KINDS
    assert set().union(*[kinds(q, x) for (q, _), x in zip(cases, want) if q == ["c", "d"]]) == ALL_KINDS
    # doc 7777 (tf 303 of c, above the 1-byte escape) holds c
    i = next(i for i, (q, d) in enumerate(cases) if q == ["c", "d"] and d[:1] == [7777])
    assert got[i][0][1] & 1 and got[i][0][0] > 0


# ---- 3. the device's own results ---------------------------------------------
def test_score_docs_equals_search(tie_ctx, indexes):  # noqa: F811
    """the top-10 of a conjunctive Search: a full mask and the same score
    bits; of a match_any Search: the same score bits"""
    import wiser_amd as w
    rng = random.Random(17)
    toks = all_tokens()
    tok = _Ctx(indexes["tok10k"][0])
    try:
        n_and = n_or = 0
        for eng, queries in ((tie_ctx.eng, TIE_QUERIES), (tok.eng, [rng.sample(toks[:200], 2) for _ in range(40)])):
            for any_ in (False, True):
                res = eng.SearchBatch([w.SearchQuery(q, n_results=10, match_any=any_) for q in queries])
                got = eng.score_docs_batch([w.SearchQuery(q, match_any=any_) for q in queries],
                                           [[e.doc_id for e in r.entries] for r in res])
                for q, r, g in zip(queries, res, got):
                    assert [s for s, _ in g] == [e.doc_score for e in r.entries], (q, any_)
                    if any_:
                        assert all(m != 0 for _, m in g)
                        n_or += len(g)
                    else:
                        assert all(m == (1 << len(q)) - 1 for _, m in g), (q, g)
                        n_and += len(g)
        assert n_and > 40 and n_or > 100
    finally:
        tok.close()


# ---- 4. the edge corpora, in every engine mode ----------------------------------
def _bucket_cases(model, n):
    rng = random.Random(3)
    queries = [["g", "s"], ["u5", "g", "y"], ["z", "y"], ["s", "z", "u7"], ["y", "g"], ["g"]]
    sparse = sorted({d for t in ("g", "s", "z", "u5", "u7") for d in model.contrib(t)})
    near = sorted({min(n - 1, max(0, d + o)) for d in sparse[::5] for o in (-1, 1)})
    docs = sparse + near + [rng.randrange(n) for _ in range(300)] + [0, n - 1]
    return [(q, docs) for q in queries]


def _doc16_cases(model, n):
    rng = random.Random(4)
    queries = [["d127", "ob"], ["s", "z"], ["t", "p", "q"], ["d2t", "f", "g"], ["d64", "d63", "z"], ["ob", "s", "t"]]
    docs = set()
    for t in ("d127", "d64", "d63", "d2t", "s", "t", "f", "g", "p", "q", "ob"):
        p = postings(model, t)
        docs.update(p[::9] + p[127::128] + p[128::128] + p[-3:] + [p[0] - 1 if p[0] else 0, min(n - 1, p[-1] + 1)])
    docs = sorted(docs) + [rng.randrange(n) for _ in range(300)] + [0, n - 1]
    return [(q, docs) for q in queries]


@pytest.mark.parametrize("corpus", ["bucket", "doc16"])
def test_score_docs_edge_corpora(built, tmp_path_factory, corpus):
    from oracle.oracle import OracleVacuum
    if corpus == "bucket":
        import bucket_corpus
        d = bucket_corpus.build_bucket_index(tmp_path_factory.mktemp("sd_bucket"))
    else:
        import doc16_corpus
        d = doc16_corpus.build_index(tmp_path_factory.mktemp("sd_doc16"))
    orc = OracleVacuum(d)
    try:
        model = OrModel(orc)
        cases = (_bucket_cases if corpus == "bucket" else _doc16_cases)(model, orc.n_docs())
        for mode in sorted(DENSE_MODES):
            eng = _engine(d, mode)
            try:
                assert check(eng, model, cases) == ALL_KINDS, mode
            finally:
                eng.close()
    finally:
        orc.close()


# ---- 5. doc-range shards --------------------------------------------------------
def test_score_docs_shards(tie_ctx, tie_cases):  # noqa: F811
    """world 3 on the tie corpus (the cuts, 6666 and 13333, fall inside
    blocks): every shard is asked every candidate; the shard that holds the doc
    answers as the unsharded engine, the others {0.0, 0}"""
    import wiser_amd as w
    from test_shard_gpu import open_shards
    from wiser_amd.shard import shard_range
    cases, want = tie_cases
    engs = open_shards(tie_ctx.eng.engine_dir_path, 3)
    try:
        ranges = [shard_range(N_TIE, r, 3) for r in range(3)]
        got = [e.score_docs_batch([w.SearchQuery(q) for q, _ in cases], [d for _, d in cases]) for e in engs]
        seen, n_out = set(), 0
        for i, ((q, docs), x) in enumerate(zip(cases, want)):
            for j, doc in enumerate(docs):
                answers = [got[r][i][j] for r in range(3)]
                owner = next(r for r, (lo, hi) in enumerate(ranges) if lo <= doc < hi)
                assert answers[owner] == x[j], (q, doc, owner, answers, x[j])
                assert all(answers[r] == (0.0, 0) for r in range(3) if r != owner), (q, doc, answers)
                # exactly one shard answers with the unsharded mask (every shard when that is 0)
                assert sum(1 for _, m in answers if m == x[j][1]) == (1 if x[j][1] else 3)
                n_out += 2
            seen |= kinds(q, x)
        assert seen == ALL_KINDS and n_out > 1000
        assert {next(r for r, (lo, hi) in enumerate(ranges) if lo <= doc < hi)
                for _, docs in cases for doc in docs} == {0, 1, 2}
    finally:
        for e in engs:
            e.close()


# ---- 6. limits and errors ---------------------------------------------------------
def _raw_call(eng, queries, off, docs):
    from wiser_amd import _capi
    n = len(queries)
    arr = (_capi.Query * max(n, 1))(*queries)
    c_off = (C.c_int64 * len(off))(*off)
    c_docs = (C.c_int32 * max(len(docs), 1))(*docs)
    out = (_capi.DocScore * max(len(docs), 1))()
    for o in out:
        o.score, o.mask = -1.0, 0xFFFF   # (a refused call must not write)
    rc = _capi.lib.wsr_score_docs(eng._h, arr, n, c_off, c_docs, out)
    return rc, [(o.score, o.mask) for o in out][:len(docs)]


def test_score_docs_errors(indexes):
    import wiser_amd as w
    from wiser_amd import _capi
    c = _Ctx(indexes["three"][0])
    try:
        eng, n = c.eng, c.eng.NumDocs()
        assert n == 3
        good = eng.resolve_terms(w.SearchQuery(["hello", "world"]))
        want = expected(c.model, ["hello", "world"], [0, 1, 2])

        def bad(**kw):
            q = eng.resolve_terms(w.SearchQuery(["hello", "world"]))
            for k, v in kw.items():
                if k == "id1":
                    q.list_ids[1] = v
                else:
                    setattr(q, k, v)
            return q

        untouched = [(-1.0, 0xFFFF)] * 3
        for q, off, docs, code in (
                (bad(n_terms=17), [0, 3], [0, 1, 2], _capi.E_LIMIT),
                (bad(flags=_capi.QUERY_PHRASE), [0, 3], [0, 1, 2], _capi.E_INVALID),
                (bad(flags=4), [0, 3], [0, 1, 2], _capi.E_INVALID),
                (bad(id1=1 << 30), [0, 3], [0, 1, 2], _capi.E_INVALID),
                (good, [0, 3], [0, -1, 2], _capi.E_INVALID),
                (good, [0, 3], [0, n, 2], _capi.E_INVALID)):
            # (the refused query second: the first one's row must stay unwritten too)
            rc, out = _raw_call(eng, [good, q], [0, 1] + off[1:], docs)
            assert rc == code and out == untouched, (q.n_terms, q.flags, docs, rc, out)
            assert _capi.lib.wsr_last_error()
        rc, out = _raw_call(eng, [good, good], [0, 2, 1], [0, 1, 2])   # a descending doc_off
        assert rc == _capi.E_INVALID and out == untouched
        with pytest.raises(_capi.WiserError) as e:   # the mirror: 17 terms
            eng.score_docs(w.SearchQuery(["hello"] * 17), [0])
        assert e.value.code == _capi.E_LIMIT
        with pytest.raises(_capi.WiserError) as e:
            eng.score_docs(w.SearchQuery(["hello", "world"], is_phrase=True), [0])
        assert e.value.code == _capi.E_INVALID
        # these succeed: nq = 0, a one-term phrase flag, WSR_QUERY_OR, k of any value, a missing term
        assert _raw_call(eng, [], [0], [])[0] == _capi.WSR_OK
        assert eng.score_docs_batch([], []) == []
        one = eng.resolve_terms(w.SearchQuery(["world"]))
        one.flags = _capi.QUERY_PHRASE
        assert _raw_call(eng, [one], [0, 3], [2, 1, 0]) == (_capi.WSR_OK, expected(c.model, ["world"], [2, 1, 0]))
        assert eng.score_docs(w.SearchQuery(["world"], is_phrase=True), [2, 1, 0]) == expected(c.model, ["world"], [2, 1, 0])
        assert eng.score_docs(w.SearchQuery(["hello"] * 16), [0, 1, 2]) == expected(c.model, ["hello"] * 16, [0, 1, 2])
        good.flags, good.k = _capi.QUERY_OR, 12345
        assert _raw_call(eng, [good], [0, 3], [0, 1, 2]) == (_capi.WSR_OK, want)
        assert eng.score_docs(w.SearchQuery(["nosuchterm", "world"]), [0, 1, 2]) == [
            (s, m << 1) for s, m in expected(c.model, ["world"], [0, 1, 2])]
        assert eng.score_docs(w.SearchQuery(["nosuchterm"]), [0, 1]) == [(0.0, 0)] * 2
        assert eng.score_docs(w.SearchQuery([]), [0, 1]) == [(0.0, 0)] * 2
        # nothing is left enqueued by the refused calls: the engine is idle and still answers
        w.sync(eng)
        assert eng.score_docs(w.SearchQuery(["hello", "world"]), [0, 1, 2]) == want
    finally:
        c.close()


# ---- 7. two threads on one handle ---------------------------------------------------
def test_score_docs_threads(tie_ctx, tie_cases):  # noqa: F811
    import wiser_amd as w
    cases, want = tie_cases
    halves = [(cases[r::2], want[r::2]) for r in range(2)]
    errors = []

    def worker(r):
        try:
            cs, ws = halves[r]
            qs, ds = [w.SearchQuery(q) for q, _ in cs], [d for _, d in cs]
            for i in range(20):
                lo = (7 * i) % len(cs)   # (calls of different sizes: the contexts' buffers grow and are reused)
                got = tie_ctx.eng.score_docs_batch(qs[lo:lo + 40], ds[lo:lo + 40])
                if got != ws[lo:lo + 40]:
                    errors.append((r, i))
        except Exception as e:   # noqa: BLE001 - surfaced below
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not errors, errors[:3]


# ---- the C++ mirror -------------------------------------------------------------------
def test_cpp_host_score_docs(indexes, tmp_path):
    """VacuumHipEngine::ScoreDocsBatch on the CLI's own results: the hits'
    score bits and full masks (tests/cpp/score_cli.cc)."""
    rng = random.Random(8)
    toks = all_tokens()
    qs = [[t] for t in rng.sample(toks, 30)] + [rng.sample(toks[:300], 2) for _ in range(60)]
    log = tmp_path / "q.log"
    log.write_text("\n".join(" ".join(q) for q in qs) + "\n")
    cli = os.path.join(ROOT, "wiser_amd", "_lib", "score_cli")
    out = subprocess.run([cli, indexes["wiki5"][0], str(log), "10"], capture_output=True, text=True,
                         check=True)
    lines = out.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == 2 * len(qs) + 1, len(lines)
    n = 0
    for i, q in enumerate(qs):
        hits = [tuple(x.split(":")) for x in lines[2 * i].split()]
        scored = [tuple(x.split(":")) for x in lines[2 * i + 1].split()]
        assert scored == [(d, s, str((1 << len(q)) - 1)) for d, s in hits], q
        n += len(hits)
    assert n > 30
