"""Test helper: the expected result of a boolean query (wsr_search_bool), from
the oracle and heapmodel alone, as or_model.py gives a disjunctive query's.

Per distinct term OrModel.contrib gives every doc's exact f64 contribution;
its keys are the term's membership.  A doc matches when every MUST slot holds
it, no MUST_NOT slot does, and at least max(min_should, 1 if no MUST else 0)
SHOULD slots do (a term given twice is two slots); its score is the sum of the
MUST and SHOULD slots that hold it, from 0.0 in query order; the matching
docs, in ascending doc id, go through heapmodel.rank_stream."""
from collections import namedtuple

from heapmodel import rank_stream

# docs held by some MUST or SHOULD slot, and why the non-matching ones fell out
# (the first rule that fails, in the order MUST, MUST_NOT, min_should)
Explain = namedtuple("Explain", "candidates lost_must lost_not lost_should matches")


class BoolModel:
    def __init__(self, or_model):
        self.m = or_model
        self.cache = {}

    def _walk(self, terms, min_should):
        """terms: [(term, role)] -> ([(score, doc)] of the matching docs in
        ascending doc id, Explain)"""
        key = (tuple(terms), min_should)
        if key in self.cache:
            return self.cache[key]
        slots = [(self.m.contrib(t) or {}, role) for t, role in terms]
        has_must = any(role == "must" for _, role in slots)
        need = max(min_should, 0 if has_must else 1)
        docs = set()
        for c, role in slots:
            if role != "must_not":
                docs.update(c)
        out, lost = [], [0, 0, 0]
        for d in sorted(docs):
            if any(role == "must" and d not in c for c, role in slots):
                lost[0] += 1
            elif any(role == "must_not" and d in c for c, role in slots):
                lost[1] += 1
            elif sum(1 for c, role in slots if role == "should" and d in c) < need:
                lost[2] += 1
            else:
                s = 0.0
                for c, role in slots:
                    if role != "must_not" and d in c:
                        s = s + c[d]
                out.append((s, d))
        self.cache[key] = (out, Explain(len(docs), lost[0], lost[1], lost[2], len(out)))
        return self.cache[key]

    def matching(self, terms, min_should=0, doc_range=None):
        m = self._walk(terms, min_should)[0]
        if doc_range is not None:
            m = [(s, d) for s, d in m if doc_range[0] <= d < doc_range[1]]
        return m

    def explain(self, terms, min_should=0):
        return self._walk(terms, min_should)[1]

    def expected(self, terms, k, min_should=0, doc_range=None):
        """-> [(score, doc)] as the engine returns them (doc_range: a doc-range
        shard's answer, the model restricted to its docs)"""
        if k <= 0:
            return []
        return rank_stream(self.matching(terms, min_should, doc_range), k)[0]
