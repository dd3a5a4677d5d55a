"""Test helper: the expected result of a disjunctive (OR) query, from the
existing oracle and heapmodel alone.

Per distinct resolved term the oracle's single-term search with k = df gives
every doc's exact f64 contribution; a doc's score is the sum of its terms'
contributions from 0.0 in query order (a repeated term is added again); the
matching docs, in ascending doc id, go through heapmodel.rank_stream (RankDoc,
then SortHeap)."""
from heapmodel import rank_stream


def or_sums(contribs):
    """contribs: per term in query order, {doc: score} (None: a missing term)
    -> [(score, doc)] in ascending doc id."""
    acc = {}
    for c in contribs:
        if not c:
            continue
        for doc, s in c.items():
            acc[doc] = acc.get(doc, 0.0) + s
    return [(acc[d], d) for d in sorted(acc)]


def or_rank(contribs, k):
    """-> [(score, doc)] as the engine returns them"""
    if k <= 0:
        return []
    return rank_stream(or_sums(contribs), k)[0]


class OrModel:
    """Expected OR results over one index; the per-term contributions and the
    per-query sums are computed once and shared."""

    def __init__(self, orc):
        self.orc = orc
        self.terms = {}
        self.sums = {}

    def contrib(self, t):
        if t not in self.terms:
            df = self.orc.df(t)
            self.terms[t] = dict(self.orc.search([t], df)[0]) if df > 0 else None
        return self.terms[t]

    def expected(self, terms, k):
        if k <= 0:
            return []
        key = tuple(terms)
        if key not in self.sums:
            self.sums[key] = or_sums([self.contrib(t) for t in terms])
        return rank_stream(self.sums[key], k)[0]
