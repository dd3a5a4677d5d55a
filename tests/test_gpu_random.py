"""Randomised GPU parity: small corpora with skewed shapes (lists of exactly
127 / 128 / 129 postings, one-posting lists, tf >= 255, empty-ish docs,
repeated terms) and random queries (1-6 terms, conjunctive or phrase,
k = 1..64) in every dense-probe mode, all against the oracle bit for bit."""
import os
import random

import pytest

from edge_corpora import write_skewed_linedoc as _corpus
from test_gpu_parity import DENSE_MODES, _engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6, 7, 8])
def test_random_corpora(tmp_path, seed):
    import wiser_amd as w
    from oracle.oracle import OracleVacuum
    ld = os.path.join(tmp_path, "c.linedoc")
    terms = _corpus(ld, seed)
    d = os.path.join(tmp_path, "idx")
    os.makedirs(d)
    w.build_from_linedoc(ld, d, "WITH_POSITIONS")
    orc = OracleVacuum(d)
    rng = random.Random(100 + seed)
    items = []
    for _ in range(1000):
        n = rng.choice([1, 1, 2, 2, 2, 3, 4, 6])
        q = [rng.choice(terms) for _ in range(n)]
        items.append((q, rng.random() < 0.4, rng.choice([1, 2, 5, 10, 10, 33, 64])))
    for mode in sorted(DENSE_MODES):
        eng = _engine(d, mode)
        res = eng.SearchBatch([w.SearchQuery(q, n_results=k, is_phrase=ph) for q, ph, k in items])
        for (q, ph, k), r in zip(items, res):
            want, dfs = orc.search(q, k, phrase=ph)
            got = [(e.doc_id, e.doc_score) for e in r.entries]
            assert got == want, (mode, q, ph, k, got[:3], want[:3])
            if want:
                assert r.doc_freqs == dfs
        eng.close()
    orc.close()
