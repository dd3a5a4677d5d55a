"""The tiny class (engine_types.h is_tiny_query; kernels.hip tiny_kernel): a
conjunctive two-term query with k <= 64 whose lists are each one decoded VInts
block runs as one wave of tiny_kernel, not as an item of segment_kernel or
lean_kernel.

The corpus's first 400 docs have one length and every query term in them has
tf 1, so all matches of a query tie and the heap's order of equal scores
decides the result.  200 more docs of five lengths hold two lists of about 100
postings with tfs 1..4, most of whose matches lie past position 64 of either
list: their scores need the right tf of the right posting of the second list
and the right doc-length code of the first.  Lists of 1, 5, 60, 127 (the largest tail) and 128 postings (one full
pack block: not a tail), placed for 0, 1 and all matches.  Every result is
compared with the oracle bit for bit (doc ids, order, f64 ==) through the C
ABI's resident batch, one query per batch and all queries in one batch, and
the batch's tiny_queries counter must equal the number of queries the rule
names, so the cases cannot pass with the path unused.
"""
import os

import pytest

from test_gpu_parity import ENGINE_ENV

pytestmark = pytest.mark.gpu

N_TIE = 400          # docs of one length, tf 1: the split corpus of test_doc_range_split
N_DOCS = 600
DOC_LEN = 24
P5 = (3, 50, 100, 126, 300)
EDGE_A = (0, 57, 199, 200, 399)
EDGE_B = (0, 123, 199, 200, 399)


def _varied_doc(i):
    """Docs 400..599: lengths 24..56, "va" (100 docs, tf 1..3) and "vb" (103 docs, tf 1..4)."""
    t = ["all"]
    if i < 520 and i % 6:
        t += ["va"] * (1 + i % 3)
    if 410 <= i < 530 and i % 7:
        t += ["vb"] * (1 + i % 4)
    n = DOC_LEN + 8 * (i % 5)
    return t + [f"z{j}" for j in range(n - len(t))]


def _doc_terms(i):
    t = ["all"]
    if i < 127:
        t += ["m127a", "m127b"]        # adjacent: the phrase "m127a m127b" occurs
    if 127 <= i < 254:
        t.append("m127c")              # no doc of m127a
    if 126 <= i < 253:
        t.append("m127d")              # one doc of m127a: 126
    if i < 128:
        t.append("f128")               # df 128: one full pack block, no tail
    if i == 5:
        t += ["s1a", "s1b"]
    if i == 200:
        t.append("s1c")
    if i in P5:
        t.append("p5")
    if i % 2 == 0:
        t.append("g2a")                # 200 postings: two blocks
    if i % 4 in (0, 1):
        t.append("g2b")
    if 10 <= i < 70:
        t.append("lo60")               # nothing in the upper half
    if i in EDGE_A:
        t.append("edgea")
    if i in EDGE_B:
        t.append("edgeb")
    return t


@pytest.fixture(scope="module")
def lab(built, tmp_path_factory):
    import wiser_amd as w
    from edge_corpora import POSITIONS_HEADER, positions_row
    from oracle.oracle import OracleVacuum
    root = str(tmp_path_factory.mktemp("tiny"))
    path = os.path.join(root, "tiny.linedoc")
    with open(path, "w") as f:
        f.write(POSITIONS_HEADER)
        for i in range(N_TIE):
            toks = _doc_terms(i)
            toks += [f"z{j}" for j in range(DOC_LEN - len(toks))]
            assert len(toks) == DOC_LEN
            f.write(positions_row(toks))
        for i in range(N_TIE, N_DOCS):
            f.write(positions_row(_varied_doc(i)))
    d = os.path.join(root, "idx")
    os.makedirs(d)
    w.build_from_linedoc(path, d, "WITH_POSITIONS")
    # dense ratio 2: a pair of lists of equal block counts is of the general
    # class, a one-block driver against "all" (4 blocks, a bitmap) is lean
    saved = {k: os.environ.get(k) for k in ENGINE_ENV}
    engines = {}
    try:
        for k in saved:
            os.environ.pop(k, None)
        os.environ["WSR_DENSE_RATIO"] = "2"
        for rng in (None, (0, 200), (200, N_TIE)):
            engines[rng] = w.VacuumEngine(d, doc_range=rng)
            engines[rng].Load()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    orc = OracleVacuum(d)
    yield engines, orc
    for e in engines.values():
        e.close()
    orc.close()


# (terms, k, phrase, tiny by the rule)
CASES = [
    (["s1a", "s1b"], 10, False, True),       # df 1 x df 1, the same doc
    (["s1a", "s1c"], 10, False, True),       # ... different docs
    (["s1c", "s1a"], 1, False, True),
    (["m127a", "m127c"], 10, False, True),   # 127 x 127: no match (the ranges do not meet)
    (["m127a", "m127d"], 10, False, True),   # one match, on the ranges' common doc
    (["m127d", "m127a"], 10, False, True),
    (["m127a", "m127b"], 1, False, True),    # all 127 match, every score equal: more matches than k
    (["m127a", "m127b"], 10, False, True),
    (["m127b", "m127a"], 10, False, True),
    (["m127a", "m127b"], 64, False, True),
    (["p5", "m127a"], 10, False, True),      # four matches: k above the match count
    (["m127a", "p5"], 64, False, True),
    (["m127a", "m127a"], 10, False, True),   # a repeated term
    (["s1a", "s1a"], 10, False, True),
    (["p5", "p5"], 3, False, True),
    (["m127c", "m127d"], 64, False, True),   # 126 matches over the upper lists
    (["lo60", "m127a"], 64, False, True),    # 60 matches
    (["va", "vb"], 10, False, True),         # varied tf and doc length, matches past position 64
    (["vb", "va"], 10, False, True),
    (["va", "vb"], 64, False, True),
    (["vb", "va"], 1, False, True),
    (["vb", "vb"], 64, False, True),
    (["f128", "m127a"], 10, False, False),   # df 128: a full pack block, not a tail
    (["m127a", "f128"], 64, False, False),
    (["f128", "f128"], 10, False, False),
    (["m127a", "m127b"], 10, True, False),   # a phrase on tiny-shaped lists
    (["m127b", "m127a"], 10, True, False),
    (["m127a", "m127b"], 65, False, False),  # k over kMaxK
    (["m127a", "m127b", "p5"], 10, False, False),
    (["p5"], 10, False, False),
]


def _run(eng, items):
    """One resident batch of items [(terms, k, phrase)] -> ([[(doc, score)]], stats, class flags)."""
    import wiser_amd as w
    from wiser_amd import _capi
    stride = max(it[1] for it in items)
    b = w.ResidentBatch(eng, len(items), stride)
    try:
        b.upload((_capi.Query * len(items))(*[
            eng.resolve(w.SearchQuery(list(t), n_results=k, is_phrase=ph))[0] for t, k, ph in items]))
        b.run()
        hits, nh = b.fetch()
        got = [[(hits[i * stride + j].doc_id, hits[i * stride + j].score) for j in range(nh[i])]
               for i in range(len(items))]
        return got, b.stats(), b.launch_class()
    finally:
        b.close()


def test_each_query_alone(lab):
    engines, orc = lab
    eng = engines[None]
    for terms, k, ph, tiny in CASES:
        got, st, _ = _run(eng, [(terms, k, ph)])
        assert got[0] == orc.search(terms, k, phrase=ph)[0], (terms, k, ph)
        assert st.tiny_queries == int(tiny), (terms, k, ph, st.tiny_queries)
        if tiny:   # every match is scored and offered to the heap: a survivor and an event
            n = len(orc.search(terms, 500)[0])
            assert (st.survivors, st.events, st.work_items) == (n, n, 1), (terms, st.survivors, st.events)


def test_all_in_one_batch(lab):
    engines, orc = lab
    got, st, _ = _run(engines[None], [c[:3] for c in CASES])
    for (terms, k, ph, _), g in zip(CASES, got):
        assert g == orc.search(terms, k, phrase=ph)[0], (terms, k, ph)
    assert st.tiny_queries == sum(c[3] for c in CASES)


def test_match_counts(lab):
    """The cases are what their comments say (from the oracle alone)."""
    _, orc = lab
    n = {tuple(t): len(orc.search(t, 500)[0]) for t in (["s1a", "s1b"], ["s1a", "s1c"], ["m127a", "m127c"],
                                                         ["m127a", "m127d"], ["m127a", "m127b"], ["p5", "m127a"])}
    assert list(n.values()) == [1, 0, 0, 1, 127, 4]
    assert [orc.df(t) for t in ("m127a", "m127b", "m127c", "m127d", "f128", "s1a", "p5")] == [127] * 4 + [128, 1, 5]
    scores = {s for _, s in orc.search(["m127a", "m127b"], 500)[0]}
    assert len(scores) == 1   # ties decide the order
    # the varied pair: tf of either list and the doc length all move the score, and most
    # matches are past position 64 of both lists
    va, vb = orc.postings("va"), orc.postings("vb")
    assert (len(va[0]), len(vb[0])) == (100, 103) and set(va[1]) == {1, 2, 3} and set(vb[1]) == {1, 2, 3, 4}
    both = sorted(set(va[0]) & set(vb[0]))
    assert len(both) > 64 and sum(va[0].index(d) >= 64 and vb[0].index(d) >= 64 for d in both) >= 20
    assert len({s for _, s in orc.search(["va", "vb"], 500)[0]}) > 20


def test_mixed_batch(lab):
    """Tiny, lean and general queries in one batch, results in query order."""
    engines, orc = lab
    items = [(["m127a", "m127b"], 10, False), (["p5", "all"], 10, False), (["g2a", "g2b"], 10, False),
             (["s1a", "s1b"], 10, False), (["all", "m127d"], 64, False), (["g2b", "g2a"], 3, False),
             (["m127a", "m127d"], 10, False), (["all"], 10, False), (["m127a", "m127b", "all"], 10, False)]
    got, st, cls = _run(engines[None], items)
    for (terms, k, ph), g in zip(items, got):
        assert g == orc.search(terms, k, phrase=ph)[0], (terms, k)
    assert cls["has_conj_lean"] and cls["has_gen"], cls
    assert st.tiny_queries == 3
    assert st.work_items - st.tiny_queries >= 6


def _in_image(orc, term, rng):
    """A one-block list has its block in the image of docs [lo, hi) when the
    block's last doc is >= lo (index.cc build_image: the first block of a list
    is never past hi), whether or not a posting of it lies in the range."""
    docs = orc.postings(term)[0]
    assert 0 < len(docs) < 128
    return docs[-1] >= rng[0]


@pytest.mark.parametrize("one_batch", [False, True])
def test_doc_range_split(lab, one_batch):
    """The corpus cut in two through the engine's doc range: a list with no
    block in the shard's image (an empty AND, not tiny), a list whose block is
    there with no posting in the range (tiny, no hit), matches on the range's
    first and last doc, and a repeated term; expected = the reference heap
    over the oracle's matches in the range."""
    from heapmodel import rank_stream
    engines, orc = lab
    queries = [(["edgea", "edgeb"], 10), (["edgeb", "edgea"], 1), (["lo60", "edgea"], 10), (["edgea", "lo60"], 64),
               (["m127a", "m127b"], 10), (["m127c", "m127d"], 64), (["edgea", "edgea"], 10), (["s1c", "edgea"], 10)]
    for rng in ((0, 200), (200, N_TIE)):
        eng = engines[rng]
        want, tiny = [], []
        for terms, k in queries:
            allm = sorted((d, s) for d, s in orc.search(terms, 500)[0] if rng[0] <= d < rng[1])
            want.append([(d, s) for s, d in rank_stream([(s, d) for d, s in allm], k)[0]])
            tiny.append(all(_in_image(orc, t, rng) for t in terms))
        # the lower image holds every list's block, the upper one drops the lists that end below it
        assert all(tiny) if rng[0] == 0 else (any(tiny) and not all(tiny))
        for edge_doc in (rng[0], rng[1] - 1):
            assert any(edge_doc in [d for d, _ in w] for w in want), edge_doc
        if one_batch:
            got, st, _ = _run(eng, [(t, k, False) for t, k in queries])
            assert got == want, rng
            assert st.tiny_queries == sum(tiny), (rng, st.tiny_queries, tiny)
        else:
            for (terms, k), w, ty in zip(queries, want, tiny):
                got, st, _ = _run(eng, [(terms, k, False)])
                assert got[0] == w, (rng, terms, k)
                assert st.tiny_queries == int(ty), (rng, terms, st.tiny_queries)
