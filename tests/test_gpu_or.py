"""GPU parity of the disjunctive (OR) queries (WSR_QUERY_OR, kernels.hip
or_kernel / or_replay_kernel) against tests/or_model.py: the oracle's exact
per-term contributions, summed per doc in query order from 0.0 and ranked by
heapmodel.rank_stream.  Doc ids, order and f64 scores must be equal; there is
no tolerance."""
import ctypes as C
import os
import random
import threading

import pytest

from conftest import all_tokens
from or_model import OrModel

pytestmark = pytest.mark.gpu


def _linedoc(path, docs):
    with open(path, "w") as f:
        f.write("FIELDS_HEADER_INDICATOR###\tdoctitle\tbody\ttokenized\n")
        for toks in docs:
            f.write(f"t\t{' '.join(toks)}\t{' '.join(toks)}\n")


def _index(tmp_path_factory, name, docs):
    import wiser_amd as w
    root = str(tmp_path_factory.mktemp(name))
    path = os.path.join(root, "c.linedoc")
    _linedoc(path, docs)
    d = os.path.join(root, "idx")
    os.makedirs(d)
    w.build_from_linedoc(path, d, "TOKEN_ONLY")
    return d


class _Ctx:
    """An engine, the oracle and the shared model of one index."""

    def __init__(self, d, positions=False):
        import wiser_amd as w
        from oracle.oracle import OracleVacuum
        self.eng = w.VacuumEngine(d, positions=positions)
        self.eng.Load()
        self.orc = OracleVacuum(d)
        self.model = OrModel(self.orc)

    def close(self):
        self.eng.close()
        self.orc.close()

    def run(self, queries, item_blocks=None):
        """queries: [(terms, k)] as OR queries in one resident batch ->
        ([[(score, doc)]], wsr_or_stats)"""
        import wiser_amd as w
        from wiser_amd import _capi
        stride = max(1, max(k for _, k in queries))
        b = w.ResidentBatch(self.eng, len(queries), stride)
        try:
            if item_blocks is not None:
                b.set_item_blocks(item_blocks)
            b.upload((_capi.Query * len(queries))(
                *[self.eng.resolve(w.SearchQuery(list(t), n_results=k, match_any=True))[0] for t, k in queries]))
            b.run()
            hits, nh = b.fetch()
            got = [[(hits[i * stride + j].score, hits[i * stride + j].doc_id) for j in range(nh[i])]
                   for i in range(len(queries))]
            return got, b.or_stats()
        finally:
            b.close()

    def check(self, queries, item_blocks=None):
        got, st = self.run(queries, item_blocks)
        bad = [(t, k, g[:3], self.model.expected(t, k)[:3]) for (t, k), g in zip(queries, got)
               if g != self.model.expected(t, k)]
        assert not bad, f"{len(bad)}/{len(queries)} OR queries differ (item_blocks={item_blocks}): {bad[:3]}"
        return st


# ---- fixtures of the suite -------------------------------------------------
def test_or_fixtures(indexes):
    import wiser_amd as w
    for name, queries in (("three", [["hello", "world"], ["world", "hello"], ["wisconsin", "big"], ["hello"],
                                     ["nosuchterm", "world"], ["big", "big", "hello"]]),
                          ("order", [["hello", "world"], ["again", "fill3"], ["fill40", "hello"], ["fill1"]])):
        c = _Ctx(indexes[name][0])
        try:
            c.check([(q, k) for q in queries for k in (1, 3, 10)])
            # the mirror: entries and doc_freqs (0 for a missing term)
            r = c.eng.Search(w.SearchQuery(queries[0] + ["nosuchterm"], n_results=3, match_any=True))
            assert [(e.doc_score, e.doc_id) for e in r.entries] == c.model.expected(queries[0], 3)
            assert r.doc_freqs == [c.orc.df(t) for t in queries[0]] + [0]
        finally:
            c.close()
    toks = all_tokens()
    rng = random.Random(21)
    c = _Ctx(indexes["tok10k"][0])
    try:
        c.check([(rng.sample(toks, rng.choice([2, 3])), k) for _ in range(200) for k in (1, 3, 10)][:600])
    finally:
        c.close()


# ---- tie corpus --------------------------------------------------------------
@pytest.fixture(scope="module")
def tie_ctx(built, tmp_path_factory):
    """test_gpu_prune.py's generator: terms a b c d, four doc lengths, tfs 1..3,
    one doc with 300 x c (a tf above 255); thousands of docs share a score."""
    rng = random.Random(5)
    docs = []
    for i in range(20000):
        toks = ["a"] * rng.choice([1, 1, 1, 2, 3])
        if rng.random() < 0.8:
            toks += ["b"] * rng.choice([1, 1, 2])
        if rng.random() < 0.5:
            toks += ["c"] * rng.choice([1, 2, 3])
        if rng.random() < 0.3:
            toks += ["d"]
        if i == 7777:
            toks += ["c"] * 300
        n = rng.choice([8, 16, 24, 64])
        toks += [f"f{j}" for j in range(max(0, n - len(toks)))]
        rng.shuffle(toks)
        docs.append(toks)
    c = _Ctx(_index(tmp_path_factory, "or_ties", docs))
    yield c
    c.close()


TIE_QUERIES = [["a", "b"], ["b", "a"], ["c", "d"], ["a", "b", "c", "d"], ["d", "d"], ["a", "zzz"],
               ["zzz", "d", "zzz"], ["zzz"], ["a", "b", "c", "d"] * 4]


@pytest.mark.parametrize("item_blocks", [63, 8, 1])
def test_or_ties(tie_ctx, item_blocks):
    """Ties at item edges: `a` has 157 blocks, so a query runs as a few items
    (63 blocks) up to 157 (one block each); k up to 64 through the running
    top-k, above it every touched doc an event and the heap in LDS."""
    st = tie_ctx.check([(q, k) for q in TIE_QUERIES for k in (1, 3, 10, 64, 65, 100, 1024)], item_blocks)
    # (["zzz"] has no item; at one block per item the 16-term query has 157 for each k)
    assert st.items >= 8 * 7 + (7 * 156 if item_blocks == 1 else 0)
    assert st.windows >= st.items and st.touched_docs >= st.events > 0


# ---- edge corpus ---------------------------------------------------------------
EDGE_TERMS = ["x", "p128", "p129", "p127", "p1", "y"]


@pytest.fixture(scope="module")
def edge_ctx(built, tmp_path_factory):
    """9,000 docs: x at every doc within 1 of a multiple of 64 (the edges of
    any power-of-two window >= 64); lists of exactly 128, 129, 127 and 1
    postings (one pack, a pack + a 1-entry VInts tail, VInts only, a single
    posting); y in the first and last two docs only."""
    n = 9000
    docs = [[f"g{i % 7}"] * (1 + i % 5) for i in range(n)]
    for i in range(n):
        if i % 64 in (63, 0, 1):
            docs[i] += ["x"] * (1 + i % 3)
    for name, cnt in (("p128", 128), ("p129", 129), ("p127", 127), ("p1", 1)):
        for j in range(cnt):
            docs[(j * n) // cnt + (cnt % 50)].append(name)
    for i in (0, 1, n - 2, n - 1):
        docs[i] += ["y", "y"]
    c = _Ctx(_index(tmp_path_factory, "or_edges", docs))
    assert [c.orc.df(t) for t in EDGE_TERMS] == [sum(1 for i in range(n) if i % 64 in (63, 0, 1)), 128, 129, 127, 1, 4]
    yield c
    c.close()


@pytest.mark.parametrize("item_blocks", [63, 1])
def test_or_edges(edge_ctx, item_blocks):
    pairs = [[a, b] for a in EDGE_TERMS for b in EDGE_TERMS if a != b]
    edge_ctx.check([(q, k) for q in pairs for k in (10, 200)], item_blocks)


# ---- MaxScore skipping -----------------------------------------------------------
@pytest.fixture(scope="module")
def skip_ctx(built, tmp_path_factory):
    """20,000 docs with `common` in every doc and `rare` in 40, spread over
    the range in four groups of ten (docs 100.., 5000.., 10000.., 15000..): a
    group fills an item's top-10 with docs that hold `rare`, whose k-th best
    is then far above common's bound, and the rare-free accumulator windows
    that follow are what the skipping jumps over."""
    rng = random.Random(8)
    docs = []
    for i in range(20000):
        toks = ["common"] * rng.choice([1, 2, 3]) + [f"f{j}" for j in range(rng.choice([3, 9, 20]))]
        docs.append(toks)
    for g in (100, 5000, 10000, 15000):
        for j in range(10):
            docs[g + 7 * j] += ["rare"] * (1 + j % 3)
    c = _Ctx(_index(tmp_path_factory, "or_skip", docs))
    assert c.orc.df("rare") == 40 and c.orc.df("common") == 20000
    yield c
    c.close()


@pytest.mark.parametrize("terms", [["common", "rare"], ["rare", "common"]])
def test_or_maxscore_skipping(skip_ctx, terms):
    st = skip_ctx.check([(terms, 10)])
    assert st.windows_skipped > 0, (st.windows, st.windows_skipped)
    st = skip_ctx.check([(terms, 65)])       # every touched doc an event: no skipping
    assert st.windows_skipped == 0 and st.touched_docs == st.events == 20000


# ---- synthetic Zipf index ----------------------------------------------------------
@pytest.fixture(scope="module")
def synth_ctx(synth_small):
    c = _Ctx(synth_small[0])
    yield c
    c.close()


def _synth_queries(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        m = rng.randint(2, 5)
        out.append([f"t{int(rng.paretovariate(0.6)) % 4000:07d}" for _ in range(m)])
    return out


def test_or_synth(synth_ctx):
    synth_ctx.check([(q, 10) for q in _synth_queries(200, 31)])


def test_or_identities(synth_ctx):
    """OR [t] is the single-term query and OR [t, t] the conjunctive [t, t],
    against the oracle directly."""
    rng = random.Random(4)
    toks = [f"t{i:07d}" for i in rng.sample(range(3000), 50)]
    for k in (10, 100):
        got, _ = synth_ctx.run([([t], k) for t in toks] + [([t, t], k) for t in toks])
        for i, t in enumerate(toks):
            assert got[i] == [(s, d) for d, s in synth_ctx.orc.search([t], k)[0]], (t, k)
            assert got[50 + i] == [(s, d) for d, s in synth_ctx.orc.search([t, t], k)[0]], (t, k)


# ---- mixed batches ------------------------------------------------------------------
def test_or_mixed_batch(positions_index):
    import wiser_amd as w
    c = _Ctx(positions_index[0], positions=True)
    try:
        rng = random.Random(12)
        words = [f"w{i}" for i in range(60)]
        items = []   # (terms, kind, k)
        for i in range(240):
            kind = ["and", "phrase", "or", "or", "k0", "missing_and", "missing_or"][i % 7]
            terms = rng.sample(words[:30], rng.randint(2, 3))
            k = 0 if kind == "k0" else rng.choice([1, 5, 10, 70])
            if kind.startswith("missing"):
                terms.insert(rng.randrange(len(terms) + 1), "nosuchword")
            items.append((terms, kind, k))
        qs = [w.SearchQuery(t, n_results=k, is_phrase=(kind == "phrase"),
                            match_any=(kind in ("or", "missing_or") or (kind == "k0" and len(t) == 3)))
              for t, kind, k in items]
        first = None
        for _ in range(2):
            res = c.eng.SearchBatch(qs)
            got = [[(e.doc_score, e.doc_id) for e in r.entries] for r in res]
            for (t, kind, k), sq, g in zip(items, qs, got):
                if k == 0:
                    want = []
                elif sq.match_any:
                    want = c.model.expected(t, k)
                else:
                    want = [(s, d) for d, s in c.orc.search(t, k, phrase=sq.is_phrase)[0]]
                assert g == want, (t, kind, k, g[:3], want[:3])
            assert first is None or got == first
            first = got
    finally:
        c.close()


def test_or_server(synth_ctx):
    import wiser_amd as w
    srv = w.Server(synth_ctx.eng, max_batch=256, window_us=300)
    items = [(q, i % 2 == 0, [1, 10, 64, 100][i % 4]) for i, q in enumerate(_synth_queries(160, 77))]
    got, errors = [None] * len(items), []

    def worker(t):
        try:
            for i in range(t, len(items), 8):
                q, any_, k = items[i]
                r = srv.Search(w.SearchQuery(q, n_results=k, match_any=any_))
                got[i] = [(e.doc_score, e.doc_id) for e in r.entries]
        except Exception as e:   # noqa: BLE001 - surfaced below
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    srv.close()
    assert not errors, errors[:3]
    for (q, any_, k), g in zip(items, got):
        want = synth_ctx.model.expected(q, k) if any_ else [(s, d) for d, s in synth_ctx.orc.search(q, k)[0]]
        assert g == want, (q, any_, k)


# ---- limits -------------------------------------------------------------------------
def test_or_errors(indexes):
    import wiser_amd as w
    from wiser_amd import _capi
    lib = _capi.lib
    eng = w.VacuumEngine(indexes["three"][0])
    eng.Load()
    try:
        with pytest.raises(_capi.WiserError) as e:
            eng.Search(w.SearchQuery(["hello"] * 17, n_results=3, match_any=True))
        assert e.value.code == _capi.E_LIMIT
        with pytest.raises(_capi.WiserError) as e:   # (loud at k = 0 too)
            eng.Search(w.SearchQuery(["hello"] * 17, n_results=0, match_any=True))
        assert e.value.code == _capi.E_LIMIT
        # the engine's own check (17 ids: the last through more_ids), and a list id past the index
        q17 = eng.resolve(w.SearchQuery(["hello"] * 17, n_results=3))[0]
        q17.flags = _capi.QUERY_OR
        assert lib.wsr_check_query(eng._h, C.byref(q17)) == _capi.E_LIMIT
        qbad = eng.resolve(w.SearchQuery(["hello", "world"], n_results=3, match_any=True))[0]
        qbad.list_ids[1] = 1 << 30
        hits1, nh1 = (_capi.Hit * 3)(), C.c_int32()
        assert lib.wsr_search_batch(eng._h, C.byref(qbad), 1, 3, hits1, C.byref(nh1)) == _capi.E_INVALID
        assert eng.Search(w.SearchQuery(["hello"] * 16, n_results=3, match_any=True)).Size() == 3
        with pytest.raises(_capi.WiserError) as e:
            eng.Search(w.SearchQuery(["hello", "world"], n_results=3, match_any=True, is_phrase=True))
        assert e.value.code == _capi.E_INVALID
        with pytest.raises(_capi.WiserError) as e:
            eng.Search(w.SearchQuery(["hello", "world"], n_results=3, match_any=True, return_snippets=True))
        assert e.value.code == _capi.E_INVALID
        q = eng.resolve(w.SearchQuery(["hello", "world"], n_results=3))[0]
        assert lib.wsr_check_query(eng._h, C.byref(q)) == _capi.WSR_OK
        for flags, rc in ((_capi.QUERY_OR, _capi.WSR_OK), (_capi.QUERY_OR | _capi.QUERY_PHRASE, _capi.E_INVALID),
                          (4, _capi.E_INVALID), (6, _capi.E_INVALID)):
            q.flags = flags
            assert lib.wsr_check_query(eng._h, C.byref(q)) == rc, flags
        # snippets: fine for the conjunctive query, refused for the disjunctive one
        buf, n = C.create_string_buffer(4096), C.c_int32()
        q.flags = 0
        assert lib.wsr_snippet(eng._h, C.byref(q), 0, 3, buf, 4096, C.byref(n)) == _capi.WSR_OK
        q.flags = _capi.QUERY_OR
        assert lib.wsr_snippet(eng._h, C.byref(q), 0, 3, buf, 4096, C.byref(n)) == _capi.E_INVALID
        # a doc-range shard step refuses a batch that holds an OR query
        b = w.ResidentBatch(eng, 2, 4)
        try:
            arr = (_capi.Query * 2)(eng.resolve(w.SearchQuery(["hello"], n_results=3))[0], q)
            b.upload(arr)
            nbytes = C.c_uint64()
            _capi.check(lib.wsr_shard_step_regions(2, 1024, C.byref(nbytes)))
            host = C.create_string_buffer(nbytes.value)
            assert lib.wsr_shard_step_emit(eng._h, b._b, 1, 2, 1024, host) == _capi.E_INVALID
            arr[1].flags = 0
            b.upload(arr)
            assert lib.wsr_shard_step_emit(eng._h, b._b, 1, 2, 1024, host) == _capi.WSR_OK
        finally:
            b.close()
    finally:
        eng.close()
