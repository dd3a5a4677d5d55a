"""Host side of the disjunctive (OR) queries: the batch former's class order
(wsr_class_order needs no handle, so no GPU) and a self-check of the tests'
OR model."""
import ctypes as C
import random

from heapmodel import rank_stream
from or_model import or_rank


def _stream(n, seed, with_or):
    from wiser_amd import _capi
    rng = random.Random(seed)
    arr = (_capi.Query * n)()
    kinds = []
    for i in range(n):
        kind = rng.choice(["and", "and", "one", "phrase", "phrase1", "or", "or"])
        arr[i].n_terms = 1 if kind in ("one", "phrase1") else rng.randint(2, 4)
        arr[i].k = 10
        arr[i].flags = {"and": 0, "one": 0, "phrase": _capi.QUERY_PHRASE, "phrase1": _capi.QUERY_PHRASE,
                        "or": _capi.QUERY_OR if with_or else 0}[kind]
        kinds.append(kind)
    return arr, kinds


def test_class_order_puts_or_queries_last(built):
    import wiser_amd as w
    arr, kinds = _stream(400, 3, with_or=True)
    order, n_conj = w.class_order(arr)
    conj = [i for i, k in enumerate(kinds) if k in ("and", "one", "phrase1")]
    phrase = [i for i, k in enumerate(kinds) if k == "phrase"]
    disj = [i for i, k in enumerate(kinds) if k == "or"]
    assert disj and phrase and conj
    assert order == conj + phrase + disj        # each class in stream order (stable)
    assert n_conj == len(conj)                  # the conjunctive class alone, as before
    # the batch former cuts every class on its own
    for batch in w.class_batches(arr, 64):
        assert len({("or" if kinds[i] == "or" else "phrase" if kinds[i] == "phrase" else "conj")
                    for i in batch}) == 1


def test_class_order_without_the_flag_is_unchanged(built):
    import wiser_amd as w
    arr, kinds = _stream(400, 3, with_or=False)
    order, n_conj = w.class_order(arr)
    conj = [i for i, k in enumerate(kinds) if k != "phrase"]
    phrase = [i for i, k in enumerate(kinds) if k == "phrase"]
    assert order == conj + phrase and n_conj == len(conj)


def test_check_query_needs_no_device_for_the_constants(built):
    from wiser_amd import _capi
    assert _capi.QUERY_OR == 2 and _capi.MAX_OR_TERMS == 16
    text = open(_capi.HEADER).read()
    assert "#define WSR_QUERY_OR 2" in text and "#define WSR_MAX_OR_TERMS 16" in text
    assert "wsr_batch_or_stats_get" in _capi.header_symbols()


def test_model_two_equal_lists_double_the_single_term_scores():
    rng = random.Random(1)
    docs = sorted(rng.sample(range(5000), 700))
    one = {d: rng.choice([0.25, 0.5, 0.75, 1.0, 1.5]) * rng.choice([1.0, 3.0]) for d in docs}
    for k in (1, 3, 10, 64, 100):
        want = rank_stream([(one[d] + one[d], d) for d in docs], k)[0]
        assert or_rank([one, one], k) == want
        # a missing term contributes nothing, wherever it stands
        assert or_rank([None, one, None, one], k) == want
    assert or_rank([None], 10) == [] and or_rank([one], 0) == []
