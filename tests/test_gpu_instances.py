"""Every lean and segment kernel instance on the edge-case corpora.

wsr_batch_upload picks the kernel instances of a batch from the batch's class
flags (plan_upload in batch_plan.cc, launch_lean): the two-term and the single-term lean
specialisations, the plain conjunctive lean instance, the two phrase lean
instances, the general kernel without / with a phrase and the wide replay.
The other parity tests send mixed batches to the corpora built to break the
lean kernel, which reach the plain instance only.  Here every instance gets
class-pure batches on those corpora -- the tie corpus (edge_corpora.py; also
written WITH_POSITIONS, "tiespos", for the phrase instances), the bucket
corpus (bucket_corpus.py), the skewed corpora of seeds 1-3 (lists of 127 /
128 / 129 postings, tf >= 255) and the large-tf corpus -- in every dense mode
and at item lengths 63, 20 and 1 where the lists are long enough.

Every case first asserts from ResidentBatch.launch_class() that the batch
selected the instance the case is named after, then compares doc ids, order
and f64 scores with OracleVacuum bit for bit, and checks from the oracle's
document frequencies that at least the expected number of work items ran.
The `mixed` cases are the control: the same queries through the plain
instance.  A case id reads <instance>-<corpus>-ib<item blocks>-<mode>.
"""
import os
from collections import namedtuple

import pytest

from test_gpu_parity import DENSE_MODES, ENGINE_ENV

pytestmark = pytest.mark.gpu

# the engine's probe structure: the three modes of test_gpu_parity.py and, on
# the bucket corpus, WSR_DENSE_DIV = 1 << 30 as test_gpu_buckets.py sets it
ENGINE_MODES = dict(DENSE_MODES, div30={"WSR_DENSE_DIV": str(1 << 30)})
POSITIONS = {"ties": False, "tiespos": True, "buckets": False, "rand1": True, "rand2": True, "rand3": True,
             "bigtf": False}
ABSENT = "absent-term"
SINGLE_WINDOWS = 8          # kSingleWindows: a single-term item spans 8 items' blocks
PHRASE_SEG_CAP = 48         # kPhraseSegCap: driver blocks per phrase item at most

# ---- the query sets ---------------------------------------------------
# (terms, k, phrase, raw): raw = (n_terms, k) overrides of the resolved query
Item = namedtuple("Item", "terms k phrase raw", defaults=(False, None))

BUCKET_US = [f"u{i}" for i in (0, 3, 7, 77, 400, 999)]    # test_gpu_buckets._queries()
TERMS = {   # the interesting terms of a corpus (conjunctive)
    "ties": ["a", "b", "c", "d"],
    "tiespos": ["a", "b", "c", "d"],
    "buckets": BUCKET_US + ["g", "s", "z", "y"],
    "rand": ["x1", "x2", "x127", "x128", "x129", "x255", "x256", "x300", "heavy", "lonely", "v0", "v1", "v4"],
    "bigtf": ["x", "y", "z", "w7", "w299"],
}
DUPLICATES = {"ties": ["a", "c"], "tiespos": ["a", "c"], "buckets": ["g", "y", "u7"], "rand": ["x128", "heavy", "v0"],
              "bigtf": ["x", "z"]}
THREE_TERMS = {"ties": ["c", "a", "b"], "tiespos": ["c", "a", "b"], "buckets": ["u7", "g", "y"],
               "rand": ["v0", "x300", "v1"], "bigtf": ["y", "z", "x"]}
PHRASE_TERMS = {"tiespos": ["a", "b", "c", "d"],
                "rand": ["v0", "v1", "v2", "heavy", "x300", "x256", "x129", "x128", "x127", "x1", "lonely"]}
PHRASE_REPEATS = {"tiespos": ["a", "c", "d"], "rand": ["v0", "heavy", "x128"]}
GENERAL_PHRASES = {
    "tiespos": [["a", "b", "a"], ["a", "a", "b"], ["b", "a", "c"], ["c", "c", "c"], ["a", "a", "a"], ["f3", "f4", "f5"],
                ["d", "d", "a"], ["c", "c", "c", "c"], ["a", "b", "c", "d"], ["b", "a", "a", "b"],
                ["a", "b", ABSENT]],
    "rand": [["v0", "v0", "v0"], ["v0", "v1", "v0"], ["v1", "v0", "v0"], ["heavy", "heavy", "heavy"],
             ["heavy", "heavy", "heavy", "heavy"], ["v0", "v0", "v1", "v0"], ["v0", "v1", "v2", "v0"],
             ["x128", "x129", "x127"], ["x300", "x300", "v0"], ["v0", "heavy", "heavy"],
             ["heavy", "heavy", "v0"], ["v0", "v1", ABSENT]],
}


def _family(corpus):
    return "rand" if corpus.startswith("rand") else corpus


def _neutral(corpus, k):
    """One empty query and one k = 0 query of three terms: both are neutral to
    the class flags (the rule reads an empty query or k <= 0 as any class)."""
    return [Item([], k), Item(THREE_TERMS[_family(corpus)], k, raw=(3, 0))]


def two_queries(corpus):
    """Every ordered pair of the interesting terms (the driver in slot 0 and in
    slot 1), duplicated terms, pairs with an absent term."""
    fam = _family(corpus)
    ts = TERMS[fam]
    qs = [[a, b] for a in ts for b in ts if a != b]
    qs += [[t, t] for t in DUPLICATES[fam]]
    qs += [[ts[0], ABSENT], [ABSENT, ts[1]]]
    return qs


def one_queries(corpus):
    return [[t] for t in TERMS[_family(corpus)]] + [[ABSENT]]


def phrase_queries(corpus):
    """Two-term phrases in both orders (some occur, some do not), repeated
    words, one with an absent term."""
    fam = _family(corpus)
    ts = PHRASE_TERMS[fam]
    qs = [[a, b] for a in ts for b in ts if a != b]
    qs += [[t, t] for t in PHRASE_REPEATS[fam]]
    qs += [[ts[0], ABSENT]]
    return qs


def batches_of(inst, corpus):
    """-> [(label, [Item])]: the batches one case of the instance runs."""
    fam = _family(corpus)
    out = []
    if inst == "two":
        for k in (1, 10, 64):
            out.append((f"k{k}", [Item(q, k) for q in two_queries(corpus)] + _neutral(corpus, k)))
        out.append(("empty", _neutral(corpus, 10) * 3))
    elif inst == "one":
        for k in (1, 10, 64, 65, 100):
            out.append((f"k{k}", [Item(q, k) for q in one_queries(corpus)] + _neutral(corpus, k)))
    elif inst == "mixed":
        for k in (1, 10, 64, 65, 100):
            qs = two_queries(corpus) + one_queries(corpus) + [THREE_TERMS[fam]]
            out.append((f"k{k}", [Item(q, k) for q in qs] + _neutral(corpus, k)))
    elif inst in ("phrase_two", "phrase_two_conj", "phrase_wide"):
        for k in (1, 10, 64):
            items = [Item(q, k, True) for q in phrase_queries(corpus)]
            if inst == "phrase_wide":
                items[3] = items[3]._replace(k=100)
            if inst == "phrase_two_conj":
                items += [Item(q, k) for q in two_queries(corpus)] + _neutral(corpus, k)
            out.append((f"k{k}", items))
    elif inst == "general_phrase":
        for k in (1, 10, 64):
            out.append((f"k{k}", [Item(q, k, True) for q in GENERAL_PHRASES[fam]]))
    elif inst == "general_conj":
        for k in (1, 10, 64):
            qs = two_queries(corpus) + [THREE_TERMS[fam]]
            out.append((f"k{k}", [Item(q, k) for q in qs] + _neutral(corpus, k)))
    else:
        raise AssertionError(inst)
    return out


# ---- what the oracle says about a batch (nothing of the engine is used) --
def live(orc, it):
    """The query reaches the kernels: k > 0 and every term in the index."""
    return it.k > 0 and it.raw is None and len(it.terms) > 0 and all(orc.df(t) > 0 for t in it.terms)


def min_items(orc, items, item_blocks):
    """Work items of the batch at least: a query's driver is its list of fewest
    128-posting blocks, and an item holds at most item_blocks of them (a
    single-term item: SINGLE_WINDOWS times as many; a phrase item: at most
    PHRASE_SEG_CAP).  The plan cuts shorter items when the other lists are
    decoded by blocks, so this is a lower bound."""
    n = 0
    for it in items:
        if not live(orc, it):
            continue
        nd = min((orc.df(t) + 127) // 128 for t in it.terms)
        phrase = it.phrase and len(it.terms) > 1
        seg = item_blocks * SINGLE_WINDOWS if len(it.terms) == 1 else (
            min(item_blocks, PHRASE_SEG_CAP) if phrase else item_blocks)
        n += (nd + seg - 1) // seg
    return n


# ---- corpora, engines and expected results, shared by every case ---------
class Lab:
    def __init__(self, tmp_path_factory):
        self.tmp = tmp_path_factory
        self.dirs, self.orcs, self.want = {}, {}, {}
        self.eng_key, self.eng = None, None

    def index(self, corpus):
        if corpus not in self.dirs:
            from bucket_corpus import build_bucket_index
            from edge_corpora import build_large_tf_index, build_skewed_index, build_tie_index
            root = self.tmp.mktemp(f"inst_{corpus}")
            if corpus in ("ties", "tiespos"):
                d = build_tie_index(root, positions=corpus == "tiespos")
            elif corpus == "buckets":
                d = build_bucket_index(root)
            elif corpus == "bigtf":
                d = build_large_tf_index(root)
            else:
                d = build_skewed_index(root, int(corpus[4:]))[0]
            self.dirs[corpus] = d
        return self.dirs[corpus]

    def oracle(self, corpus):
        if corpus not in self.orcs:
            from oracle.oracle import OracleVacuum
            self.orcs[corpus] = OracleVacuum(self.index(corpus))
        return self.orcs[corpus]

    def expected(self, corpus, it):
        """The oracle's result, asked once per distinct (terms, k, phrase)."""
        if it.raw is not None or it.k <= 0 or not it.terms:
            return []
        key = (corpus, tuple(it.terms), it.k, bool(it.phrase))
        if key not in self.want:
            self.want[key] = self.oracle(corpus).search(list(it.terms), it.k, phrase=it.phrase)[0]
        return self.want[key]

    def n_matches_over(self, corpus, it, n):
        """More than n docs match the query (the oracle asked for n + 1)."""
        return len(self.expected(corpus, it._replace(k=n + 1))) > n

    def open_engine(self, corpus):
        """A loaded engine over the corpus's whole index (the mode's environment is set)."""
        import wiser_amd as w
        e = w.VacuumEngine(self.index(corpus), positions=POSITIONS[corpus])
        e.Load()
        return e

    def engine(self, corpus, mode):
        """One engine at a time: the cases are ordered by (corpus, mode)."""
        if self.eng_key != (corpus, mode):
            self.close_engine()
            saved = {k: os.environ.get(k) for k in ENGINE_ENV}
            try:
                for k in saved:
                    os.environ.pop(k, None)
                os.environ.update(ENGINE_MODES[mode])
                e = self.open_engine(corpus)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            self.eng_key, self.eng = (corpus, mode), e
        return self.eng

    def close_engine(self):
        if self.eng is not None:
            self.eng.close()
        self.eng_key, self.eng = None, None

    def close(self):
        self.close_engine()
        for o in self.orcs.values():
            o.close()


@pytest.fixture(scope="module")
def lab(built, tmp_path_factory):
    lb = Lab(tmp_path_factory)
    yield lb
    lb.close()


# ---- the flags an instance's batch must show ------------------------------
# after the upload (they select the kernel instances); True / False = must be
# set / clear, absent = not part of the instance's definition
SELECT = {
    "two": dict(two_conj=True, one_conj=False, has_phrase=False, has_wide=False, has_or=False),
    "one": dict(two_conj=False, one_conj=True, has_phrase=False, has_gen=False, has_conj_lean=True, has_or=False),
    "mixed": dict(two_conj=False, one_conj=False, has_phrase=False, has_conj_lean=True, has_or=False),
    "phrase_two": dict(has_phrase=True, two_ph=True, has_wide=False, has_conj_lean=False, has_or=False),
    "phrase_two_conj": dict(has_phrase=True, two_ph=True, two_conj=True, one_conj=False, has_wide=False,
                            has_or=False),
    "phrase_wide": dict(has_phrase=True, two_ph=False, has_wide=True, has_conj_lean=False, has_or=False),
    "general_phrase": dict(has_phrase=True, two_ph=True, gen_phrase=True, has_gen=True, has_conj_lean=False,
                           has_or=False),
    "general_conj": dict(two_conj=False, one_conj=False, has_phrase=False, has_gen=True, has_conj_lean=False,
                         has_or=False),
}
LEAN = ("two", "one", "mixed", "phrase_two", "phrase_two_conj", "phrase_wide")


def selected(inst, label, mode, cls):
    """The flags of the upload that differ from what the instance's batch must
    select (empty: the case runs the instance it is named after)."""
    want = dict(SELECT[inst])
    if inst in ("one", "mixed"):
        want["has_wide"] = label in ("k65", "k100")
    if label == "empty":   # no query reaches a kernel: neither class holds an item
        want.update(has_conj_lean=False, has_gen=False)
    elif mode == "blocks":
        # no bitmaps or buckets: a query of several terms is of the general class
        if inst in ("two", "phrase_two", "phrase_two_conj", "phrase_wide"):
            want.update(has_gen=True, has_conj_lean=False)
        if inst.startswith("phrase"):
            want["gen_phrase"] = True
    else:
        # every list of these corpora that a query probes carries a bitmap or
        # buckets: a query of one or two terms is lean
        if inst in ("two", "phrase_two_conj"):
            want.update(has_conj_lean=True, has_gen=False)
        if inst in ("phrase_two", "phrase_two_conj", "phrase_wide"):
            want.update(gen_phrase=False)
        if inst in ("phrase_two", "phrase_wide"):
            want.update(has_gen=False)
    return {f: (cls[f], v) for f, v in want.items() if cls[f] != v}


def ran(inst, cls):
    """ran_conj / ran_gen of the run that differ from the launch rule: a batch
    with phrases launches the conjunctive lean kernel and the general kernel
    only for the classes the upload found; any other batch launches both."""
    want = {"ran_conj": not cls["has_phrase"] or cls["has_conj_lean"],
            "ran_gen": not cls["has_phrase"] or cls["has_gen"]}
    return {f: (cls[f], v) for f, v in want.items() if cls[f] != v}


# ---- the cases -----------------------------------------------------------
Case = namedtuple("Case", "inst corpus ib mode")
ITEM_BLOCKS = {"ties": (63, 20, 1), "tiespos": (63, 20, 1), "buckets": (63, 20, 1)}   # (else 63: short lists)
MODES_3 = ("blocks", "dense", "dense_all")


def _cases():
    out = []
    for corpus in POSITIONS:
        modes = MODES_3 + (("div30",) if corpus == "buckets" else ())
        for mode in modes:
            for ib in ITEM_BLOCKS.get(corpus, (63,)):
                insts = []
                if corpus != "tiespos":   # (its conjunctive cases run on "ties")
                    insts += ["two", "one", "mixed"]
                if POSITIONS[corpus]:
                    insts += ["phrase_two", "phrase_two_conj", "phrase_wide"]
                out += [Case(i, corpus, ib, mode) for i in insts]
            # the general class: item length 63 (the plan cuts its items by cost)
            if POSITIONS[corpus]:
                out.append(Case("general_phrase", corpus, 63, mode))
            if mode == "blocks" and corpus != "tiespos":
                out.append(Case("general_conj", corpus, 63, mode))
    return out


CASES = _cases()


def _raw_query(eng, it):
    import wiser_amd as w
    src = it if it.raw is None else it._replace(k=1)
    q = eng.resolve(w.SearchQuery(list(src.terms), n_results=src.k, is_phrase=src.phrase))[0]
    if it.raw is not None:
        assert q.n_terms == len(it.terms), "the k = 0 query's terms must resolve"
        q.n_terms, q.k = it.raw
    return q


@pytest.mark.parametrize("case", CASES, ids=["-".join((c.inst, c.corpus, f"ib{c.ib}", c.mode)) for c in CASES])
def test_instance(lab, case):
    import wiser_amd as w
    from wiser_amd import _capi
    inst, corpus, ib, mode = case
    orc = lab.oracle(corpus)
    eng = lab.engine(corpus, mode)
    for label, items in batches_of(inst, corpus):
        stride = max(1, max(it.k for it in items))
        b = w.ResidentBatch(eng, len(items), stride)
        try:
            b.set_item_blocks(ib)
            b.upload((_capi.Query * len(items))(*[_raw_query(eng, it) for it in items]))
            cls = b.launch_class()
            assert not selected(inst, label, mode, cls), (label, cls)   # {flag: (got, want)}
            b.run()
            hits, nh = b.fetch()
            cls = b.launch_class()
            assert not ran(inst, cls), (label, cls)
            bad = []
            for i, it in enumerate(items):
                got = [(hits[i * stride + j].doc_id, hits[i * stride + j].score) for j in range(nh[i])]
                want = lab.expected(corpus, it)
                if got != want:
                    bad.append((it.terms, it.k, it.phrase, got[:3], want[:3]))
            assert not bad, f"{inst} {label} ib={ib} {mode}: {len(bad)}/{len(items)} differ, first: {bad[:3]}"
            # non-vacuity, from the oracle alone
            n_live = [it for it in items if live(orc, it)]
            if label == "empty":
                assert not n_live and not any(nh[i] for i in range(len(items)))
            else:
                assert n_live
            st = b.stats()
            need = min_items(orc, items, ib)
            assert st.work_items >= need, (label, st.work_items, need)
            if inst in ("general_phrase", "general_conj"):
                # the general kernel did the work: every live query is of its
                # class, so the driver blocks are its own; other_blocks counts
                # the blocks it decoded from the other lists, which it does
                # only where they carry no bitmap or buckets to probe
                assert st.driver_blocks > 0
                if mode == "blocks":
                    assert st.other_blocks > 0
            if corpus in ("ties", "tiespos") and inst in ("two", "one") and n_live:
                deep = sum(lab.n_matches_over(corpus, it, it.k) for it in n_live)
                assert 2 * deep >= len(n_live), (label, deep, len(n_live))
            phrases = [it for it in items if it.phrase]
            if phrases:
                hit = sum(bool(lab.n_matches_over(corpus, it, 0)) for it in phrases)
                assert 3 * hit >= len(phrases) and hit < len(phrases), (label, hit, len(phrases))
        finally:
            b.close()


def test_item_arithmetic(lab):
    """The item lengths do what the cases rely on: on the tie corpus the driver
    of ["a", "b"] has 125 blocks, so item lengths 63, 20 and 1 give 2, 7 and
    125 items (7 items of 20 blocks: long enough for the in-flight floor
    refresh every 8 blocks; 1: every item a single block, none replayed
    fused), and the engine cuts exactly those for a lean query."""
    import wiser_amd as w
    from wiser_amd import _capi
    orc = lab.oracle("ties")
    assert (min(orc.df("a"), orc.df("b")) + 127) // 128 == 125
    eng = lab.engine("ties", "dense_all")
    items = [Item(["a", "b"], 10)]
    for ib, n in ((63, 2), (20, 7), (1, 125)):
        assert min_items(orc, items, ib) == n
        b = w.ResidentBatch(eng, 1, 10)
        try:
            b.set_item_blocks(ib)
            b.upload((_capi.Query * 1)(_raw_query(eng, items[0])))
            cls = b.launch_class()
            assert cls["two_conj"] and cls["has_conj_lean"] and not cls["has_gen"], cls
            b.run()
            b.fetch()
            assert b.stats().work_items == n, (ib, b.stats().work_items)
        finally:
            b.close()
