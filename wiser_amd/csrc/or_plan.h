// The item cutting and event-slot sizing of one disjunctive traversal, shared
// by the upload plan's WSR_QUERY_OR queries (batch_plan.cc) and the boolean
// queries' plan (bool_plan.cc).  Pure host, no HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "batch_plan.h"
#include "engine_types.h"

namespace wiser {

// How many blocks of L can hold a doc of [lo, hi) (lo < hi): from the first
// block whose last doc is >= lo to the first whose last doc is >= hi - 1.
inline uint32_t blocks_overlapping(const ImageView& v, const ListDev& L, uint32_t lo, uint32_t hi) {
  // first block of L whose last doc is >= x (nblk: none)
  auto first_block = [&](uint32_t x) {
    const BlockDev* b0 = v.blocks + L.blk0;
    return static_cast<uint32_t>(
        std::lower_bound(b0, b0 + L.nblk, x, [](const BlockDev& e, uint32_t w) { return e.last < w; }) - b0);
  };
  const uint32_t f = first_block(lo);
  return f < L.nblk ? std::min(first_block(hi - 1), L.nblk - 1) - f + 1 : 0u;
}

// The MaxScore bounds of the query's scoring slots (bit t of `scoring`), summed
// in ascending (bound, slot) order into oq->ubsum; 0.0 for the other slots.
inline void sum_maxscore_bounds(const ImageView& v, uint32_t scoring, OrQuery* oq) {
  int by[kMaxOrTerms];
  int ns = 0;
  for (int t = 0; t < oq->nt; ++t) {
    oq->ubsum[t] = 0.0;
    if ((scoring >> t) & 1u) by[ns++] = t;
  }
  auto ub = [&](int t) { return 2.2 * v.lists[oq->list[t]].idf; };
  std::stable_sort(by, by + ns, [&](int a, int c) { return ub(a) < ub(c); });
  double sum = 0.0;
  for (int r = 0; r < ns; ++r) {
    sum += ub(by[r]);
    oq->ubsum[by[r]] = sum;
  }
}

// The plan of one disjunctive query (its resolved terms in oq->list; bit t of
// `scoring`: slot t carries a MaxScore bound, sum_maxscore_bounds): the
// image's doc range cut into items at the last doc of every s-th block of the
// query's longest list, s chosen so that an item carries about `target` blocks
// over all its lists (doc ids spread alike over the lists' blocks), and each
// item's event slot sized for its worst case -- every doc of its range an
// event, or every posting of the blocks that overlap it.  Appends the items
// and advances *ev_total.
inline void plan_or_query(const ImageView& v, uint32_t target, OrQuery* oq, std::vector<OrItem>* items,
                          uint64_t* ev_total, uint32_t scoring = ~0u) {
  const int nt = oq->nt;
  sum_maxscore_bounds(v, scoring, oq);
  uint64_t total = 0;
  int lg = 0;
  uint32_t top = 0;   // one past the last doc of its lists in the image
  for (int t = 0; t < nt; ++t) {
    const ListDev& L = v.lists[oq->list[t]];
    total += L.nblk;
    if (L.nblk > v.lists[oq->list[lg]].nblk) lg = t;
    top = std::max(top, L.last + 1);
  }
  const ListDev& G = v.lists[oq->list[lg]];
  const uint32_t step = static_cast<uint32_t>(std::max<uint64_t>(1, uint64_t{target} * G.nblk / total));
  const uint32_t img_lo = v.doc_lo, img_hi = std::min(v.doc_hi, top);
  auto last_of = [&](const ListDev& L, uint32_t j) { return v.blocks[L.blk0 + j].last; };
  oq->item_base = static_cast<uint32_t>(items->size());
  for (uint32_t j0 = 0; j0 < G.nblk; j0 += step) {
    const uint32_t j1 = std::min(j0 + step, G.nblk);
    const uint32_t lo = std::max(img_lo, j0 ? last_of(G, j0 - 1) + 1 : 0u);
    const uint32_t hi = j1 == G.nblk ? img_hi : std::min(img_hi, last_of(G, j1 - 1) + 1);
    if (lo >= hi) continue;
    uint64_t blocks = 0;
    for (int t = 0; t < nt; ++t) blocks += blocks_overlapping(v, v.lists[oq->list[t]], lo, hi);
    if (!blocks) continue;
    OrItem it{};
    it.oq = 0;   // (set by the caller: the query's place in its table)
    it.doc_lo = lo;
    it.doc_hi = hi;
    it.ev_cap = static_cast<uint32_t>(std::min<uint64_t>(hi - lo, 128 * blocks));
    it.ev_base = *ev_total;
    *ev_total += it.ev_cap;
    items->push_back(it);
  }
  oq->n_items = static_cast<uint32_t>(items->size()) - oq->item_base;
}

}  // namespace wiser
