"""Every lean and segment kernel instance over doc-range shards of the
edge-case corpora.

test_gpu_instances.py pins every kernel instance on the whole image.  A
doc-range shard runs the same lean, segment and replay kernels over an image
with doc_lo > 0, whose bitmaps and buckets cover the shard's span only and
whose edge blocks also hold postings outside the range; the worker that ends a
query reduces its events (EventFilter) into an owner's slot instead of writing
hits, and the owner replay kernel (narrow and wide) rebuilds the reference heap
from every shard's events.  Here the class-pure batches of
test_gpu_instances.py (batches_of) go through one shard step
(test_shard_gpu.run_step_items) over tilings of the same corpora, and every
query's owner result must equal OracleVacuum.search on the WHOLE index: doc
ids, order and f64 scores, bit for bit.

The cuts: the even 2-way and 3-way splits (w2, w3) of every corpus; on the tie
corpus (ties, tiespos) the 4-way tiling [0,128) [128,7777) [7777,7778)
[7778,20000) (hand4: "a" is in every doc, so doc 128 opens its second block --
a boundary on a block edge; the third shard is doc 7777 alone, c's tf 303); on
rand1 a 3-way tiling whose middle shard lies in the widest gap between two
neighbouring postings of x127 / x128 / x129 (gap: the shard's image holds an
edge block of that list with no posting in range), computed from the oracle's
postings.

The product that runs (a case id reads
<instance>-<corpus>-<cut>-ib<item blocks>-<mode>):
  * mode dense: every instance x every cut of its corpora x the item lengths
    63, 20 and 1 on ties / tiespos / buckets (63 elsewhere; the general
    instances: 63, as in test_gpu_instances.py);
  * modes blocks and dense_all: every instance on the 2-way split, all its
    item lengths;
  * general_conj exists in mode blocks only: there on every cut.
The corpora: ties, buckets, bigtf for the conjunctive instances, tiespos for
the phrase instances, rand1 for all.

Every case asserts, per shard and from ResidentBatch.launch_class(), the class
flags that do not depend on the image; the image-dependent ones (has_gen,
has_conj_lean, gen_phrase) per shard in mode blocks, from the oracle's
postings, and otherwise that at least one shard ran the named instance with
items; that no owner's fetch reports an error; the parity above; and, from the
oracle alone, that the case is not vacuous (queries match in several shards,
at least the expected number of work items ran in every shard).

test_deferred_owner_replay_ties sends the two-term and single-term tie batches
through wsr_shard_steps with the default deferral (the owner replay of an
earlier step group in the lean kernel's tail).
"""
import os
from bisect import bisect_left
from collections import namedtuple

import pytest

from test_gpu_instances import (ENGINE_MODES, ITEM_BLOCKS, POSITIONS, SELECT, SINGLE_WINDOWS, Lab, _neutral, _raw_query,
                                batches_of, live, selected)
from test_gpu_parity import ENGINE_ENV
from test_shard_gpu import open_shards, run_step_items

pytestmark = pytest.mark.gpu

IMAGE_FLAGS = ("has_gen", "has_conj_lean", "gen_phrase")   # may differ between the shards of a case
FIXED_FLAGS = ("two_conj", "one_conj", "has_phrase", "two_ph", "has_wide", "has_or")
assert all(f in FIXED_FLAGS + IMAGE_FLAGS for want in SELECT.values() for f in want)
TIE_TERMS = set("abcd")
HAND4 = [(0, 128), (128, 7777), (7777, 7778), (7778, 20000)]
GAP_LISTS = ("x127", "x128", "x129")


# ---- what the oracle says about a shard (nothing of the engine is used) ---
def image_blocks(docs, lo, hi):
    """The 128-posting blocks of a list (its doc ids: docs) in the image of the
    shard [lo, hi): block r holds docs in (last of block r - 1, its last], and
    is loaded when that interval can meet the range (block 0: whenever its last
    doc is not below lo) -- the loader's rule (build_image)."""
    out = []
    for r in range((len(docs) + 127) // 128):
        last = docs[min(len(docs), 128 * r + 128) - 1]
        if (r == 0 or docs[128 * r - 1] + 1 < hi) and last >= lo:
            out.append(r)
    return out


def widest_gap_cut(orc, n_docs):
    """-> (term, [(lo, hi)] * 3): the middle shard fills the widest gap between
    two neighbouring postings of one of GAP_LISTS."""
    best = None
    for t in GAP_LISTS:
        docs = orc.postings(t)[0]
        for a, b in zip(docs, docs[1:]):
            if best is None or b - a > best[0]:
                best = (b - a, t, a + 1, b)
    _, t, lo, hi = best
    return t, [(0, lo), (lo, hi), (hi, n_docs)]


class ShardLab(Lab):
    """Lab with the shard engines of one (corpus, cut, mode) open at a time."""

    def __init__(self, tmp_path_factory):
        super().__init__(tmp_path_factory)
        self.sh_key, self.sh = None, []
        self.all, self.docs, self.cuts = {}, {}, {}

    def matches(self, corpus, it):
        """Every doc the query matches, sorted (the oracle asked for n_docs)."""
        key = (corpus, tuple(it.terms), bool(it.phrase))
        if key not in self.all:
            orc = self.oracle(corpus)
            self.all[key] = sorted(d for d, _ in orc.search(list(it.terms), orc.n_docs(), phrase=it.phrase)[0])
        return self.all[key]

    def n_in(self, corpus, it, rg):
        """Docs of the shard [lo, hi) the query matches."""
        m = self.matches(corpus, it)
        return bisect_left(m, rg[1]) - bisect_left(m, rg[0])

    def postings(self, corpus, term):
        """The list's doc ids (ascending)."""
        if (corpus, term) not in self.docs:
            self.docs[corpus, term] = self.oracle(corpus).postings(term)[0]
        return self.docs[corpus, term]

    def postings_in(self, corpus, term, rg):
        docs = self.postings(corpus, term)
        return bisect_left(docs, rg[1]) - bisect_left(docs, rg[0])

    def in_image(self, corpus, it, rg):
        """Every list of the (live) query has a block in the shard's image."""
        return all(image_blocks(self.postings(corpus, t), *rg) for t in it.terms)

    def ranges(self, corpus, cut):
        if (corpus, cut) not in self.cuts:
            from wiser_amd.shard import shard_range
            orc = self.oracle(corpus)
            n = orc.n_docs()
            if cut in ("w2", "w3"):
                rgs = [shard_range(n, r, int(cut[1])) for r in range(int(cut[1]))]
            elif cut == "hand4":
                assert n == HAND4[-1][1], "the tie corpus changed: the hand-made tiling no longer covers it"
                rgs = HAND4
            else:
                t, rgs = widest_gap_cut(orc, n)
                lo, hi = rgs[1]
                docs = self.postings(corpus, t)
                # the property the cut exists for
                assert lo < hi and image_blocks(docs, lo, hi) and not any(lo <= d < hi for d in docs), (t, rgs)
            self.cuts[corpus, cut] = [tuple(r) for r in rgs]
        return self.cuts[corpus, cut]

    def open_shard_engines(self, corpus, rgs):
        """The loaded shard engines of the tiling rgs (the mode's environment is set)."""
        return open_shards(self.index(corpus), len(rgs), positions=POSITIONS[corpus], ranges=rgs)

    def shards(self, corpus, cut, mode):
        if self.sh_key != (corpus, cut, mode):
            self.close_shards()
            rgs = self.ranges(corpus, cut)
            saved = {k: os.environ.get(k) for k in ENGINE_ENV}
            try:
                for k in saved:
                    os.environ.pop(k, None)
                os.environ.update(ENGINE_MODES[mode])
                self.sh = self.open_shard_engines(corpus, rgs)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            self.sh_key = (corpus, cut, mode)
        return self.sh

    def close_shards(self):
        for e in self.sh:
            e.close()
        self.sh_key, self.sh = None, []

    def close(self):
        self.close_shards()
        super().close()


@pytest.fixture(scope="module")
def lab(built, tmp_path_factory):
    lb = ShardLab(tmp_path_factory)
    yield lb
    lb.close()


# ---- the cases -------------------------------------------------------------
Case = namedtuple("Case", "inst corpus cut ib mode")
CONJ = ("two", "one", "mixed")
PHRASE = ("phrase_two", "phrase_two_conj", "phrase_wide")
CORPORA = {"ties": CONJ, "tiespos": PHRASE, "buckets": CONJ, "rand1": CONJ + PHRASE, "bigtf": CONJ}
CUTS = {"ties": ("w2", "w3", "hand4"), "tiespos": ("w2", "w3", "hand4"), "buckets": ("w2", "w3"),
        "rand1": ("w2", "w3", "gap"), "bigtf": ("w2", "w3")}


def _cases():
    out = []
    for corpus, insts in CORPORA.items():
        for cut in CUTS[corpus]:
            for mode in ("dense", "blocks", "dense_all"):
                if mode == "dense" or cut == "w2":
                    for ib in ITEM_BLOCKS.get(corpus, (63,)):
                        out += [Case(i, corpus, cut, ib, mode) for i in insts]
                    if POSITIONS[corpus]:
                        out.append(Case("general_phrase", corpus, cut, 63, mode))
                if mode == "blocks" and corpus != "tiespos":
                    out.append(Case("general_conj", corpus, cut, 63, mode))
    return out   # (ordered by (corpus, cut, mode): one set of shard engines open at a time)


CASES = _cases()


def image_flags_in_blocks_mode(lab, corpus, items, rg):
    """Mode blocks, no bitmaps or buckets: a query of several terms is of the
    general class wherever it is live in the shard, a single-term one lean."""
    orc = lab.oracle(corpus)
    here = [it for it in items if live(orc, it) and lab.in_image(corpus, it, rg)]
    return {"has_gen": any(len(it.terms) > 1 for it in here),
            "has_conj_lean": any(len(it.terms) == 1 for it in here),
            "gen_phrase": any(len(it.terms) > 1 and it.phrase for it in here)}


def check_non_vacuous(lab, case, label, items, rgs, runs):
    """From the oracle alone (and the shards' work item counts)."""
    inst, corpus, cut, ib, mode = case
    orc = lab.oracle(corpus)
    alive = [it for it in items if live(orc, it)]
    if label == "empty":
        assert not alive and not any(r.stats.work_items for r in runs)
        return
    assert alive
    if corpus in ("ties", "tiespos"):
        # every live query over a, b, c, d matches in every shard (hand4: but
        # the one-doc shard).  Of the phrases: the two-term ones that occur at
        # all ("d d" never does, d's tf is 1; the longer ones are too rare for
        # a shard of 128 docs)
        for it in alive:
            if set(it.terms) <= TIE_TERMS and (not it.phrase or (len(it.terms) == 2 and lab.matches(corpus, it))):
                for rg in rgs:
                    assert rg == (7777, 7778) or lab.n_in(corpus, it, rg), \
                        f"the tie corpus changed: {it.terms} (phrase {it.phrase}) has no match in {rg}"
    else:
        spread = [it for it in alive if sum(bool(lab.n_in(corpus, it, rg)) for rg in rgs) >= 2]
        assert spread, f"no live query of {inst} {label} matches in two shards of {rgs}"
    for rg, r in zip(rgs, runs):
        need = sum(bool(lab.n_in(corpus, it, rg)) for it in alive)
        assert r.stats.work_items >= need, (label, rg, r.stats.work_items, need)
    if inst == "one" and ib == 1 and corpus == "ties" and cut == "w2":
        # the floor-seed case: items beyond the first of a single-term query in every shard
        for rg, r in zip(rgs, runs):
            need = sum(-(-lab.postings_in(corpus, it.terms[0], rg) // (128 * SINGLE_WINDOWS)) for it in alive)
            assert need >= 2 * len(alive), (rg, need)
            assert r.stats.work_items >= need, (label, rg, r.stats.work_items, need)
    phrases = [it for it in items if it.phrase]
    if phrases:
        hit = sum(bool(lab.matches(corpus, it)) for it in phrases)
        assert 3 * hit >= len(phrases) and hit < len(phrases), (label, hit, len(phrases))


@pytest.mark.parametrize("case", CASES,
                         ids=["-".join((c.inst, c.corpus, c.cut, f"ib{c.ib}", c.mode)) for c in CASES])
def test_shard_instance(lab, case):
    inst, corpus, cut, ib, mode = case
    rgs = lab.ranges(corpus, cut)
    engs = lab.shards(corpus, cut, mode)
    for label, items in batches_of(inst, corpus):
        k_pad = min(it.k for it in items)   # (k <= every k of the batch: neutral to has_wide too)
        got, runs, rcs = run_step_items(engs, items, ib, _neutral(corpus, k_pad))
        assert not any(rcs), (label, rcs)   # an error flag of the step fails the owner's fetch
        # selection
        ran_named = False
        for rg, r in zip(rgs, runs):
            diff = selected(inst, label, mode, r.cls)   # {flag: (got, want)} against the whole image's
            assert not {f: v for f, v in diff.items() if f in FIXED_FLAGS}, (label, rg, diff)
            if label == "empty":
                assert not diff, (label, rg, diff)
            elif mode == "blocks":
                want = image_flags_in_blocks_mode(lab, corpus, items, rg)
                assert {f: r.cls[f] for f in want} == want, (label, rg, r.cls, want)
            ran_named = ran_named or (not diff and r.stats.work_items > 0 and r.stats.driver_blocks > 0)
        assert ran_named or label == "empty", (label, [(r.cls, r.stats.work_items) for r in runs])
        # parity with the whole index
        bad = []
        for it, g in zip(items, got):
            want = lab.expected(corpus, it)
            if g != want:
                bad.append((it.terms, it.k, it.phrase, g[:3], want[:3]))
        assert not bad, f"{inst} {label} {cut} ib={ib} {mode}: {len(bad)}/{len(items)} differ, first: {bad[:3]}"
        check_non_vacuous(lab, case, label, items, rgs, runs)


@pytest.mark.parametrize("world", [2, 3])
def test_deferred_owner_replay_ties(lab, monkeypatch, world):
    """The lean kernel's tail replays the owned queries of an earlier step
    group (wsr_shard_steps, OwnerJob): the two-term and single-term tie batches,
    k = 1, 10 and 64, each a step group of its own through LoopbackGroup /
    NativeShardedSearcher with the default deferral, so that every group but
    the last ones has its replay taken by a later group's lean kernel; then the
    same groups again, each batch stepped while its replay may be pending.
    Every rank's owned slice equals the oracle on the whole index."""
    import wiser_amd as w
    from wiser_amd import _capi
    from wiser_amd.shard import LoopbackGroup, NativeShardedSearcher, slot_for_fill
    monkeypatch.delenv("WSR_REPLAY_DEFER", raising=False)
    for k in ENGINE_ENV:
        monkeypatch.delenv(k, raising=False)
    lab.close_shards()
    d = lab.index("ties")
    sets = []
    for inst in ("two", "one"):
        for label, items in batches_of(inst, "ties"):
            if label in ("k1", "k10", "k64"):
                sets.append(list(items))
    n = max(len(s) for s in sets)
    n += -n % world
    for s in sets:   # one q_per_owner for every batch: padded with neutral queries, none dropped
        pad = _neutral("ties", s[0].k)
        s += [pad[i % 2] for i in range(n - len(s))]
    qpr = n // world
    exp = [[lab.expected("ties", it) for it in s] for s in sets]
    assert all(sum(bool(e) for e in es) >= 4 for es in exp)   # (a, b, c and d at least: no batch is empty)
    L = LoopbackGroup(world)
    S = [NativeShardedSearcher(d, r, world, share_id=None, loopback=L, positions=False) for r in range(world)]
    bs = []
    try:
        for s in S:
            row = []
            for items in sets:
                b = w.ResidentBatch(s.engine, n, max(it.k for it in items))
                row.append(b)
                b.upload((_capi.Query * n)(*[_raw_query(s.engine, it) for it in items]))
            bs.append(row)
        # the slot from a first pass
        for i in range(len(sets)):
            for r, s in enumerate(S):
                s.steps([bs[r][i]], qpr, 1 << 20)
        slot = slot_for_fill(max(s.max_fill(bs[r][i]) for r, s in enumerate(S) for i in range(len(sets))), qpr)
        before = S[0].comm_stats()["replays_in_lean"]
        for _ in range(2):
            for i in range(len(sets)):
                for r, s in enumerate(S):   # every rank submits the group before the next group
                    s.steps([bs[r][i]], qpr, slot)
        for r, s in enumerate(S):
            for i, items in enumerate(sets):
                b = bs[r][i]
                hits, nh = s.fetch_owned(b, qpr)
                got = [[(hits[q * b.stride + j].doc_id, hits[q * b.stride + j].score) for j in range(nh[q])]
                       for q in range(qpr)]
                want = exp[i][r * qpr:(r + 1) * qpr]
                bad = [(items[r * qpr + q].terms, g[:3], e[:3]) for q, (g, e) in enumerate(zip(got, want)) if g != e]
                assert not bad, f"world {world} rank {r} batch {i}: {len(bad)}/{qpr} differ, first: {bad[:3]}"
        assert S[0].comm_stats()["replays_in_lean"] > before   # the deferred path ran
    finally:
        for row in bs:
            for b in row:
                b.close()
        for s in S:
            s.close()
        L.close()
