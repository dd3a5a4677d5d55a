"""The bloom-pruned phrase paths on the edge corpora: every phrase kernel
instance, whole image and doc-range shards, on indexes written with the
two-way phrase bloom filters.

An engine opened with bloom_factor > 0 on such an index loads every posting's
two filters (HostImage::blm, 32 bytes per posting slot) and prunes with them
before the exact position check, as the reference does
(QueryProcessor::IsPossibleToPresent, query_processing.h:766-884): phrase_match2
in the lean two-term phrase instance, phrase_match / bloom_possible in the
general kernel.  Honest filters have no false negatives, so a kernel that reads
another posting's filter, the other side or none at all gives the right result
on an honest index.  Here the class-pure phrase batches of test_gpu_instances.py
(batches_of) run on the tie corpus and the skewed corpus of seed 1, both written
with filters, honest and tampered (bloom_tamper.py: the filters of chosen boxes
of 128 postings taken away, which makes the reference prune docs that do hold
the phrase): the engine must prune exactly the docs the reference prunes.

Expected results: OracleVacuum(index, bloom_factor=f).search on the WHOLE
index -- doc ids, order and f64 scores, compared by equality.

A corpus key reads <corpus>_<honest|tampered>_f<bloom factor>; a case id
<instance>-<key>-ib<item blocks>-<mode>, the shard cases with the cut
(test_gpu_shard_instances.py: w2, w3, hand4, gap) after the key.

Whole image:
  * honest, factor 1, and tampered, factors 1 and 3: modes blocks, dense and
    dense_all x item lengths 63, 20 and 1 on the tie corpus (63 on rand1;
    general_phrase: 63, the plan cuts its items by cost);
  * tampered tie corpus, factor 0 (BLOOM_NEVER_USE: no filters are built, the
    exact results): mode dense, item length 63.
Shards:
  * honest, factor 1: w2 in mode dense (item lengths 63 and 1 on the tie
    corpus);
  * tampered, factors 1 and 3, mode dense: the tie corpus over w2, w3 and
    hand4 with item lengths 63 and 1 (hand4: box 0 of "a" is shard 0 and box 1
    opens shard 1, both blanked), rand1 over w3 and gap; modes blocks and
    dense_all: w2, item length 63.

Every case asserts that launch_class() selected the named instance, the parity
above, that at least the expected work items ran, that the engine did load the
filters (image_info()["pos_bytes"] above that of a factor-0 engine of the same
index and range) and, over shards, that no owner's fetch reports an error.

The tests without the gpu mark need the oracle alone: the honest filters change
no result; the tampering changes at least one in ten of the live phrase queries
at factors 1 and 3, and at least one in ten of those still have hits (a kernel
that drops every doc of a tampered list is wrong too); the side rule
(CheckBloomWithEnableFactor: term 0's next filter when f * df0 <= df1, term 1's
prior filter when f * df1 < df0, else none) takes every branch on the tie
corpus; the changed phrases match, and lose docs, in several shards of every
cut.
"""
import os
from collections import namedtuple

import pytest

from bloom_tamper import tampered_copy
from conftest import BLOOM_ENTRIES, BLOOM_RATIO
from test_gpu_instances import MODES_3, _neutral, _raw_query, batches_of, live, min_items, ran, selected
from test_gpu_shard_instances import FIXED_FLAGS, ShardLab, image_flags_in_blocks_mode
from test_shard_gpu import open_shards, run_step_items

gpu = pytest.mark.gpu

INSTANCES = ("phrase_two", "phrase_two_conj", "phrase_wide", "general_phrase")
Key = namedtuple("Key", "corpus variant factor")   # corpus: tiespos / rand1; variant: honest / tampered


def key_id(key):
    return f"{key.corpus}_{key.variant}_f{key.factor}"


class BloomLab(ShardLab):
    """ShardLab over corpus keys: the index of (corpus, variant), the oracle
    and the engines of (corpus, variant, factor)."""

    def __init__(self, tmp_path_factory):
        super().__init__(tmp_path_factory)
        self.blanked, self.pos0 = {}, {}

    def index(self, key):
        ik = (key.corpus, key.variant)
        if ik not in self.dirs:
            from edge_corpora import build_skewed_index, build_tie_index
            hk = (key.corpus, "honest")
            if hk not in self.dirs:
                root = self.tmp.mktemp(f"bloom_{key.corpus}")
                bloom = (BLOOM_RATIO, BLOOM_ENTRIES)
                self.dirs[hk] = (build_tie_index(root, positions=True, bloom=bloom) if key.corpus == "tiespos"
                                 else build_skewed_index(root, int(key.corpus[4:]), bloom=bloom)[0])
            if key.variant == "tampered":
                dst = os.path.join(os.path.dirname(self.dirs[hk]), "idx_tampered")
                self.blanked[key.corpus] = tampered_copy(self.dirs[hk], dst, key.corpus)
                self.dirs[ik] = dst
        return self.dirs[ik]

    def oracle(self, key):
        if key not in self.orcs:
            from oracle.oracle import OracleVacuum
            self.orcs[key] = OracleVacuum(self.index(key), bloom_factor=key.factor)
            assert self.orcs[key].has_bloom()
        return self.orcs[key]

    def open_engine(self, key):
        import wiser_amd as w
        e = w.VacuumEngine(self.index(key), positions=True, bloom_factor=key.factor)
        e.Load()
        return e

    def open_shard_engines(self, key, rgs):
        return open_shards(self.index(key), len(rgs), positions=True, ranges=rgs, bloom_factor=key.factor)

    def pos_bytes0(self, key, rg=None):
        """image_info()["pos_bytes"] of a factor-0 engine (it builds no
        filters) of the key's index, whole or the shard rg; opened once."""
        ck = (key.corpus, key.variant, rg)
        if ck not in self.pos0:
            import wiser_amd as w
            e = w.VacuumEngine(self.index(key), positions=True, bloom_factor=0, doc_range=rg)
            e.Load()
            try:
                self.pos0[ck] = e.image_info()["pos_bytes"]
            finally:
                e.close()
            assert self.pos0[ck] > 0
        return self.pos0[ck]


@pytest.fixture(scope="module")
def lab(built, tmp_path_factory):
    lb = BloomLab(tmp_path_factory)
    yield lb
    lb.close()


def check_filters_loaded(lab, key, eng, rg=None):
    got, none = eng.image_info()["pos_bytes"], lab.pos_bytes0(key, rg)
    if key.factor:
        assert got > none, (key, rg, got, none)
    else:
        assert got == none, (key, rg, got, none)


# ---- the cases ---------------------------------------------------------------
TIE_H, RAND_H = Key("tiespos", "honest", 1), Key("rand1", "honest", 1)
TIE_T = {f: Key("tiespos", "tampered", f) for f in (0, 1, 3)}
RAND_T = {f: Key("rand1", "tampered", f) for f in (1, 3)}
LEAN_PHRASE = INSTANCES[:3]
WholeCase = namedtuple("WholeCase", "inst key ib mode")
ShardCase = namedtuple("ShardCase", "inst key cut ib mode")


def _whole_cases():
    out = []
    for key in (TIE_H, RAND_H, TIE_T[1], TIE_T[3], RAND_T[1], RAND_T[3]):
        for mode in MODES_3:
            for ib in (63, 20, 1) if key.corpus == "tiespos" else (63,):
                out += [WholeCase(i, key, ib, mode) for i in LEAN_PHRASE]
            out.append(WholeCase("general_phrase", key, 63, mode))
    out += [WholeCase(i, TIE_T[0], 63, "dense") for i in INSTANCES]
    return out   # (ordered by (key, mode): one engine open at a time)


# the tampered shard cuts in mode dense, and their item lengths
TAMPERED_CUTS = {"tiespos": ("w2", "w3", "hand4"), "rand1": ("w3", "gap")}
SHARD_ITEM_BLOCKS = {"tiespos": (63, 1), "rand1": (63,)}


def _shard_cases():
    def group(key, cut, mode, ibs):
        return [ShardCase(i, key, cut, ib, mode) for ib in ibs for i in LEAN_PHRASE] + [
            ShardCase("general_phrase", key, cut, 63, mode)]
    out = []
    for key in (TIE_H, RAND_H):
        out += group(key, "w2", "dense", SHARD_ITEM_BLOCKS[key.corpus])
    for key in (TIE_T[1], TIE_T[3], RAND_T[1], RAND_T[3]):
        for cut in TAMPERED_CUTS[key.corpus]:
            out += group(key, cut, "dense", SHARD_ITEM_BLOCKS[key.corpus])
        for mode in ("blocks", "dense_all"):
            out += group(key, "w2", mode, (63,))
    return out   # (ordered by (key, cut, mode): one set of shard engines open at a time)


WHOLE, SHARD = _whole_cases(), _shard_cases()


def parity(lab, key, items, got):
    """-> the items whose result is not the oracle's: doc ids, order, f64 scores"""
    bad = []
    for it, g in zip(items, got):
        want = lab.expected(key, it)
        if g != want:
            bad.append((it.terms, it.k, it.phrase, g[:3], want[:3]))
    return bad


@gpu
@pytest.mark.parametrize("case", WHOLE, ids=["-".join((c.inst, key_id(c.key), f"ib{c.ib}", c.mode)) for c in WHOLE])
def test_bloom_instance(lab, case):
    import wiser_amd as w
    from wiser_amd import _capi
    inst, key, ib, mode = case
    orc = lab.oracle(key)
    eng = lab.engine(key, mode)
    check_filters_loaded(lab, key, eng)
    for label, items in batches_of(inst, key.corpus):
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
            got = [[(hits[i * stride + j].doc_id, hits[i * stride + j].score) for j in range(nh[i])]
                   for i in range(len(items))]
            bad = parity(lab, key, items, got)
            assert not bad, f"{inst} {key_id(key)} {label} ib={ib} {mode}: {len(bad)}/{len(items)} differ, " \
                            f"first: {bad[:3]}"
            assert any(live(orc, it) for it in items)
            st = b.stats()
            need = min_items(orc, items, ib)
            assert st.work_items >= need, (label, st.work_items, need)
            if inst == "general_phrase":
                assert st.driver_blocks > 0
        finally:
            b.close()


@gpu
@pytest.mark.parametrize("case", SHARD,
                         ids=["-".join((c.inst, key_id(c.key), c.cut, f"ib{c.ib}", c.mode)) for c in SHARD])
def test_bloom_shard_instance(lab, case):
    inst, key, cut, ib, mode = case
    orc = lab.oracle(key)
    rgs = lab.ranges(key, cut)
    engs = lab.shards(key, cut, mode)
    for rg, e in zip(rgs, engs):
        check_filters_loaded(lab, key, e, rg)
    for label, items in batches_of(inst, key.corpus):
        k_pad = min(it.k for it in items)
        got, runs, rcs = run_step_items(engs, items, ib, _neutral(key.corpus, k_pad))
        assert not any(rcs), (label, rcs)   # an error flag of the step fails the owner's fetch
        ran_named = False
        for rg, r in zip(rgs, runs):
            diff = selected(inst, label, mode, r.cls)   # {flag: (got, want)} against the whole image's
            assert not {f: v for f, v in diff.items() if f in FIXED_FLAGS}, (label, rg, diff)
            if mode == "blocks":
                want = image_flags_in_blocks_mode(lab, key, items, rg)
                assert {f: r.cls[f] for f in want} == want, (label, rg, r.cls, want)
            ran_named = ran_named or (not diff and r.stats.work_items > 0 and r.stats.driver_blocks > 0)
        assert ran_named, (label, [(r.cls, r.stats.work_items) for r in runs])
        bad = parity(lab, key, items, got)
        assert not bad, f"{inst} {key_id(key)} {label} {cut} ib={ib} {mode}: {len(bad)}/{len(items)} differ, " \
                        f"first: {bad[:3]}"
        # every shard ran an item at least for each query the (pruning) oracle matches there
        alive = [it for it in items if live(orc, it)]
        assert alive
        for rg, r in zip(rgs, runs):
            need = sum(bool(lab.n_in(key, it, rg)) for it in alive)
            assert r.stats.work_items >= need, (label, rg, r.stats.work_items, need)


# ---- what the oracle alone says about the cases (no GPU) -----------------------
def phrase_items(corpus):
    """The distinct (terms, k) phrases of several terms in the instances' batches."""
    seen = {}
    for inst in INSTANCES:
        for _, items in batches_of(inst, corpus):
            for it in items:
                if it.phrase and len(it.terms) > 1 and it.raw is None:
                    seen.setdefault((tuple(it.terms), it.k), it)
    return list(seen.values())


def results(lab, key, it):
    return lab.oracle(key).search(list(it.terms), it.k, phrase=True)[0]


@pytest.mark.parametrize("key", [TIE_H, RAND_H], ids=key_id)
def test_honest_filters_change_no_result(lab, key):
    """No false negatives: the pruning oracle equals the exact one."""
    exact = key._replace(factor=0)
    items = phrase_items(key.corpus)
    assert sum(bool(results(lab, exact, it)) for it in items) * 3 >= len(items)
    for it in items:
        assert results(lab, key, it) == results(lab, exact, it), it


@pytest.mark.parametrize("key", [TIE_T[1], TIE_T[3], RAND_T[1], RAND_T[3]], ids=key_id)
def test_tampering_changes_results(lab, key):
    from oracle.oracle import bloom_stats
    exact = key._replace(factor=0)
    alive = [it for it in phrase_items(key.corpus) if live(lab.oracle(exact), it)]
    _, pruned0 = bloom_stats()
    now = [results(lab, key, it) for it in alive]
    _, pruned1 = bloom_stats()
    assert pruned1 > pruned0
    diff = [r for r, it in zip(now, alive) if r != results(lab, exact, it)]
    hit = [r for r in diff if r]
    assert 10 * len(diff) >= len(alive), (len(diff), len(alive))
    assert 10 * len(hit) >= len(diff), (len(hit), len(diff))


def side_taken(f, df0, df1):
    """CheckBloomWithEnableFactor (query_processing.h:796-807)"""
    return "term 0 next" if f * df0 <= df1 else "term 1 prior" if f * df1 < df0 else "none"


def test_side_rule_coverage(lab):
    sides = {}
    for f in (1, 3):
        orc = lab.oracle(TIE_T[f])
        two = [it for it in phrase_items("tiespos") if len(it.terms) == 2 and live(orc, it)]
        sides[f] = {tuple(it.terms): side_taken(f, orc.df(it.terms[0]), orc.df(it.terms[1])) for it in two}
    assert {"term 0 next", "term 1 prior"} <= set(sides[1].values())
    assert {"term 0 next", "term 1 prior", "none"} <= set(sides[3].values())
    assert sides[3]["a", "b"] == "none"
    # and the side matters: some phrase's result at factor 3 is not that at factor 1
    assert any(results(lab, TIE_T[1], it) != results(lab, TIE_T[3], it) for it in phrase_items("tiespos"))


SHARD_CUTS = sorted({(c.key, c.cut) for c in SHARD if c.key.variant == "tampered"})


@pytest.mark.parametrize("key,cut", SHARD_CUTS, ids=[f"{key_id(k)}-{c}" for k, c in SHARD_CUTS])
def test_changed_phrases_span_shards(lab, key, cut):
    """The phrases the tampering changes match in two shards of the cut at
    least, and the docs they lose lie in two shards at least: one of them is an
    image whose lists start past their first box."""
    exact = key._replace(factor=0)
    rgs = lab.ranges(key, cut)
    alive = [it for it in phrase_items(key.corpus) if live(lab.oracle(exact), it)]
    changed = [it for it in alive if lab.matches(key, it) != lab.matches(exact, it)]
    assert changed
    assert any(sum(bool(lab.n_in(key, it, rg)) for rg in rgs) >= 2 for it in changed)
    losing = {i for it in changed for i, rg in enumerate(rgs) if lab.n_in(key, it, rg) < lab.n_in(exact, it, rg)}
    assert len(losing) >= 2 and max(losing) > 0, losing
