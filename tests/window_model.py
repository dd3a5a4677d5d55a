"""Test helper: a model of the window schedule of the disjunctive traversal
(OR and boolean queries), written from DESIGN 4j / 4l / 4o.  It does not model
scores -- those come from OrModel / BoolModel's per-term contributions -- only
which windows of one work item run, which are jumped over, which docs are
touched and which become events.

One item is the doc range [doc_lo, doc_hi) of one query:

* The essential set starts as all scoring slots: the lead alone when the query
  has a MUST term (no MaxScore runs then), the SHOULD slots otherwise.
* The next window is the aligned 2,048-doc window of the smallest unconsumed
  posting over the essential slots, clipped to the item.
* With a doc set, a window that holds no doc of the set in range is passed
  over: it counts neither as run nor as skipped.  (The host first cuts a
  filtered query's items to the set's first and last doc, DESIGN 4o: the
  caller passes the cut range, and windows outside it count nowhere.)
* In a run window every posting of every slot (MUST_NOT slots included) is
  touched; the matching docs pass in doc order to the item's running top-k, and
  the insertions (heapmodel.rank_stream) are the item's events.
* After each run window theta is the k-th best score the item has passed on;
  a scoring slot whose ubsum -- the bounds 2.2 * idf summed in ascending
  (bound, slot) order -- is <= 0.998 * theta stops being essential.  A slot can
  come back only if theta could fall, which it cannot.
* k > 64: nothing is skipped and every matching doc is an event.
* windows_skipped: the aligned windows between the end of the last window
  handled and the start of the next one (or the item's end), counted up to the
  window that holds the last posting, in the image, of any scoring slot that
  is non-essential at that moment ("Statistics").
"""
from collections import namedtuple

from heapmodel import rank_stream

WINDOW = 2048
MARGIN = 0.998
MAX_NARROW_K = 64
BLOCK = 128   # postings per block of a list

Schedule = namedtuple("Schedule", "windows skipped passed touched events stages run_bases stream")


def list_end(postings, doc_lo=0, doc_hi=None):
    """One past the last doc of a list's blocks in the image of [doc_lo,
    doc_hi) (a shard keeps whole blocks: block r holds the docs (last of block
    r - 1, last of block r]); 0: no block overlaps the range.  postings: the
    list's doc ids in ascending order."""
    end = 0
    for r in range(0, len(postings), BLOCK):
        last = postings[min(r + BLOCK, len(postings)) - 1]
        below_hi = r == 0 or doc_hi is None or postings[r - 1] + 1 < doc_hi
        if below_hi and last >= doc_lo:
            end = last + 1
    return end


def bound_sums(bounds, scoring, order="ascending", names=None):
    """ubsum per slot (0.0 for a slot that is not scoring).  order "query" and
    names (a repeated name counted once) are the deliberately wrong variants."""
    by = [t for t in range(len(bounds)) if scoring[t]]
    if order == "ascending":
        by.sort(key=lambda t: (bounds[t], t))
    out, total, seen = [0.0] * len(bounds), 0.0, {}
    for t in by:
        if names is not None and names[t] in seen:
            out[t] = seen[names[t]]
            continue
        total += bounds[t]
        out[t] = total
        if names is not None:
            seen[names[t]] = total
    return out


def walk(contribs, roles, bounds, k, doc_lo, doc_hi, min_should=0, docset=None, ends=None, skipping=True,
         order="ascending", names=None):
    """contribs: per slot in query order {doc: f64} (a MUST_NOT slot's values
    are not read); roles: "must" / "should" / "must_not" per slot; bounds:
    2.2 * idf per slot; ends: list_end per slot (None: one past the slot's
    last doc); docset: a set of doc ids or None -> Schedule"""
    nt = len(contribs)
    ends = ends or [max(c) + 1 if c else 0 for c in contribs]
    posts = [sorted(d for d in c if doc_lo <= d < doc_hi) for c in contribs]
    musts = [t for t in range(nt) if roles[t] == "must"]
    shoulds = [t for t in range(nt) if roles[t] == "should"]
    nots = [t for t in range(nt) if roles[t] == "must_not"]
    need = max(min_should, 0 if musts else 1)
    led = bool(musts)
    if led:
        lead = min(musts, key=lambda t: ((len(contribs[t]) + BLOCK - 1) // BLOCK, t))
        ess = {lead}
    else:
        ess = set(shoulds)
    ubsum = bound_sums(bounds, [roles[t] != "must_not" for t in range(nt)], order, names)
    narrow = k <= MAX_NARROW_K
    at = [0] * nt   # per slot: its first posting not below pos

    windows = skipped = passed = touched = 0
    stages, run_bases, stream = [len(ess)], [], []
    pos = doc_lo
    while pos < doc_hi:
        for t in range(nt):
            while at[t] < len(posts[t]) and posts[t][at[t]] < pos:
                at[t] += 1
        nxt = min([posts[t][at[t]] for t in ess if at[t] < len(posts[t])], default=doc_hi)
        base = nxt - nxt % WINDOW
        lo = max(base, pos)
        # the windows jumped over while a non-essential scoring list still has postings
        open_end = max([ends[t] for t in shoulds if not led and t not in ess and ends[t] > pos], default=0)
        end = min(doc_hi if nxt >= doc_hi else lo, open_end)
        if end > pos:
            skipped += -(-(end - pos) // WINDOW)
        if nxt >= doc_hi:
            break
        hi = min(base + WINDOW, doc_hi)
        if docset is not None and not any(d in docset for d in range(lo, hi)):
            passed += 1
            pos = hi
            continue
        windows += 1
        run_bases.append(base)
        held = {}
        for t in range(nt):
            j = at[t]
            while j < len(posts[t]) and posts[t][j] < lo:
                j += 1
            while j < len(posts[t]) and posts[t][j] < hi:
                held.setdefault(posts[t][j], []).append(t)
                j += 1
        touched += len(held)
        for d in sorted(held):
            h = held[d]
            if any(t not in h for t in musts) or any(t in h for t in nots):
                continue
            if sum(1 for t in h if roles[t] == "should") < need:
                continue
            if docset is not None and d not in docset:
                continue
            s = 0.0
            for t in h:   # (query order)
                if roles[t] != "must_not":
                    s = s + contribs[t][d]
            stream.append((s, d))
        pos = hi
        if skipping and not led and narrow and len(stream) >= k:
            theta = sorted((s for s, _ in stream), reverse=True)[k - 1]
            ess = {t for t in shoulds if not ubsum[t] <= MARGIN * theta}
            if len(ess) != stages[-1]:
                stages.append(len(ess))
    events = len(rank_stream(stream, k)[1]) if narrow else len(stream)
    return Schedule(windows, skipped, passed, touched, events, stages, run_bases, stream)
