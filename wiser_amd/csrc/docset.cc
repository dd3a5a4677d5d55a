// Doc sets (include/wiser_hip.h, wsr_docset): a bitmap over the whole index's
// doc ids resident in HBM, built from ids on the host (wsr_docset_from_ids) or
// from a boolean query on the device (wsr_docset_from_bool: match_set_kernel),
// and the two calls that read one per query as a filter:
// wsr_search_bool_filtered (bool_filtered_kernel, then or_replay_kernel) and
// wsr_count_bool_filtered (count_filtered_kernel).  The plans are plan_bool's
// and plan_count's as they are; the sets go to the device as a table of
// bitmap pointers beside the BoolRoles table, one entry per planned query.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bool_plan.h"
#include "engine_impl.h"

using namespace wiser;

namespace {

// words of a bitmap over n_docs docs, padded to whole windows (at least one)
size_t docset_words(int64_t n_docs) {
  const size_t windows = std::max<size_t>(1, (static_cast<size_t>(n_docs) + kOrWindow - 1) / kOrWindow);
  return windows * (kOrWindow / 32);
}

// filters[0 .. nq) belong to h (NULL entries and a NULL array are fine)
int check_filters(const wsr_handle* h, const wsr_docset* const* filters, int32_t nq, std::string* err) {
  if (!filters) return WSR_OK;
  for (int32_t i = 0; i < nq; ++i)
    if (filters[i] && filters[i]->h != h) {
      *err = "query " + std::to_string(i) + ": the doc set was made on another handle";
      return WSR_E_INVALID;
    }
  return WSR_OK;
}

bool any_filter(const wsr_docset* const* filters, int32_t nq) {
  if (!filters) return false;
  for (int32_t i = 0; i < nq; ++i)
    if (filters[i]) return true;
  return false;
}

// The call's queries with those whose set is empty turned into queries without
// terms, which the plan settles; null when no set is empty.  (Only after the
// plan of the queries as given has passed every check.)
std::vector<wsr_bool_query> without_empty_sets(const wsr_bool_query* q, int32_t nq,
                                               const wsr_docset* const* filters) {
  std::vector<wsr_bool_query> out;
  for (int32_t i = 0; i < nq; ++i)
    if (filters[i] && filters[i]->count == 0) {
      if (out.empty()) out.assign(q, q + nq);
      out[i].n_terms = 0;
    }
  return out;
}

// The plan's side of the filters: table[i] = the bitmap of planned query i
// (NULL: none), and every item's doc range cut to the docs its query's set can
// hold (an item left without docs runs no window).
void apply_filters(BoolPlan* p, const wsr_docset* const* filters, std::vector<const uint32_t*>* table) {
  table->assign(p->qs.size(), nullptr);
  for (size_t i = 0; i < p->qs.size(); ++i) {
    const wsr_docset* s = filters[p->qs[i].q];
    if (!s) continue;
    (*table)[i] = s->bits.get();
    const OrQuery& oq = p->qs[i];
    for (uint32_t j = 0; j < oq.n_items; ++j) {
      OrItem& it = p->items[oq.item_base + j];
      it.doc_lo = std::max(it.doc_lo, s->lo);
      it.doc_hi = std::max(it.doc_lo, std::min(it.doc_hi, s->hi));
    }
  }
}

// wsr_count_bool_ex over plan p with the filter table (one entry per planned
// query); out_bits: the bitmap of wsr_docset_from_bool (out_words words,
// zeroed here on the call's stream), or null.  counts[0 .. nq) receives every
// query's count.
int run_count(wsr_handle* h, const BoolPlan& p, const std::vector<const uint32_t*>& table, int32_t nq,
              int64_t* counts, uint32_t* out_bits, size_t out_words, wsr_or_stats* stats) {
  const size_t n_q = p.qs.size(), n_items = p.items.size();
  std::unique_ptr<CountCtx> c = h->count_pool.take();
  uint32_t ctr[kNumCounters];
  unsigned long long sv[kNumOrStats];
  std::vector<uint32_t> icnt(n_items);
  try {
    HIP_OK(hipSetDevice(h->device));
    if (!c) {
      c.reset(new CountCtx());
      c->st = gpu::make_stream();
      c->d_ctr.alloc(kNumCounters);
      c->d_stats.alloc(kNumOrStats);
    }
    if (n_q > c->d_qs.size()) gpu::alloc_group(n_q + n_q / 4, c->d_qs, c->d_roles);
    if (n_items > c->d_items.size()) gpu::alloc_group(n_items + n_items / 4 + 64, c->d_items, c->d_icnt);
    c->d_filt.reserve(n_q, n_q + n_q / 4);
    const hipStream_t st = c->st;
    HIP_OK(hipMemcpyAsync(c->d_qs, p.qs.data(), sizeof(OrQuery) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_roles, p.roles.data(), sizeof(BoolRoles) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_filt, table.data(), sizeof(const uint32_t*) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_items, p.items.data(), sizeof(OrItem) * n_items, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(c->d_ctr, 0, sizeof(uint32_t) * kNumCounters, st));
    HIP_OK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * kNumOrStats, st));
    HIP_OK(hipMemsetAsync(c->d_icnt, 0, sizeof(uint32_t) * n_items, st));
    if (out_bits) HIP_OK(hipMemsetAsync(out_bits, 0, sizeof(uint32_t) * out_words, st));
    HIP_OK(launch_count_items_filtered(h->args, c->d_qs, c->d_roles, c->d_filt, c->d_items,
                                       static_cast<uint32_t>(n_items), p.nt_max, c->d_icnt, out_bits, c->d_ctr,
                                       c->d_stats, st));
    HIP_OK(hipMemcpyAsync(ctr, c->d_ctr, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(sv, c->d_stats, sizeof sv, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(icnt.data(), c->d_icnt, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (const std::exception& e) {
    // (the context goes with what it holds, once its stream is idle)
    if (c && c->st) (void)hipStreamSynchronize(c->st);
    return fail(WSR_E_HIP, e.what());
  }
  h->count_pool.give(std::move(c));
  if (ctr[kCtrError]) return fail(WSR_E_INTERNAL, "device reported error flags " + std::to_string(ctr[kCtrError]));
  for (int32_t i = 0; i < nq; ++i) counts[i] = 0;   // (the queries settled on the host)
  for (const OrQuery& oq : p.qs) {
    int64_t sum = 0;
    for (uint32_t j = 0; j < oq.n_items; ++j) sum += icnt[oq.item_base + j];
    counts[oq.q] = sum;
  }
  if (stats) *stats = or_stats_of(sv);
  return WSR_OK;
}

// a new set on h with a bitmap of the index's size, not yet filled
std::unique_ptr<wsr_docset> new_set(wsr_handle* h) {
  std::unique_ptr<wsr_docset> s(new wsr_docset());
  s->h = h;
  s->bits.alloc(docset_words(h->idx.n_docs()));
  return s;
}

}  // namespace

extern "C" int wsr_docset_from_ids(wsr_handle* h, const int32_t* docs, int64_t n, wsr_docset** out) {
  if (!h || !out || n < 0 || (n > 0 && !docs)) return fail(WSR_E_INVALID, "null argument");
  const int64_t n_docs = h->idx.n_docs();
  for (int64_t i = 0; i < n; ++i)
    if (docs[i] < 0 || docs[i] >= n_docs)
      return fail(WSR_E_INVALID, "doc " + std::to_string(i) + ": id " + std::to_string(docs[i]) +
                                     " outside the index's " + std::to_string(n_docs) + " docs");
  std::vector<uint32_t> bits(docset_words(n_docs), 0u);
  uint32_t lo = 0xFFFFFFFFu, hi = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t d = static_cast<uint32_t>(docs[i]);
    bits[d >> 5] |= 1u << (d & 31u);
    lo = std::min(lo, d);
    hi = std::max(hi, d + 1u);
  }
  int64_t count = 0;
  for (const uint32_t w : bits) count += __builtin_popcount(w);
  try {
    HIP_OK(hipSetDevice(h->device));
    std::unique_ptr<wsr_docset> s = new_set(h);
    HIP_OK(hipMemcpy(s->bits, bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice));
    s->count = count;
    s->lo = count ? lo : 0u;
    s->hi = count ? hi : 0u;
    *out = s.release();
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

extern "C" int wsr_docset_from_bool(wsr_handle* h, const wsr_bool_query* q, const wsr_docset* within,
                                    int32_t item_blocks, wsr_docset** out) {
  if (!h || !q || !out) return fail(WSR_E_INVALID, "null argument");
  if (item_blocks < 0 || item_blocks > kSegCost) return fail(WSR_E_INVALID, "item blocks must be 0..63");
  if (within && within->h != h) return fail(WSR_E_INVALID, "the doc set was made on another handle");
  BoolPlan p;
  std::string why;
  const uint32_t target = item_blocks ? static_cast<uint32_t>(item_blocks) : h->args.seg_cap;
  const int prc = plan_count(h->view(), q, 1, true, target, &p, &why);
  if (prc) return fail(prc, why);
  const bool settled = p.items.empty() || (within && within->count == 0);
  std::vector<const uint32_t*> table;
  if (!settled) apply_filters(&p, &within, &table);
  std::unique_ptr<wsr_docset> s;
  try {
    HIP_OK(hipSetDevice(h->device));
    s = new_set(h);
    if (settled) {   // the empty set
      HIP_OK(hipMemset(s->bits, 0, s->bits.bytes()));
      HIP_OK(hipStreamSynchronize(nullptr));
    }
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  if (!settled) {
    if (p.items.size() > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "over 2^32 boolean work items");
    int64_t count = 0;
    const int rc = run_count(h, p, table, 1, &count, s->bits, s->bits.size(), nullptr);
    if (rc) return rc;
    s->count = count;
    if (count) {
      s->lo = h->args.doc_lo;
      s->hi = h->args.doc_hi;
      if (within) {
        s->lo = std::max(s->lo, within->lo);
        s->hi = std::max(s->lo, std::min(s->hi, within->hi));
      }
    }
  }
  *out = s.release();
  return WSR_OK;
}

extern "C" int wsr_docset_count(wsr_handle* h, const wsr_docset* s, int64_t* n) {
  if (!h || !s || !n) return fail(WSR_E_INVALID, "null argument");
  if (s->h != h) return fail(WSR_E_INVALID, "the doc set was made on another handle");
  *n = s->count;
  return WSR_OK;
}

extern "C" int wsr_docset_ids(wsr_handle* h, const wsr_docset* s, int32_t* out, int64_t cap, int64_t* n) {
  if (!h || !s || !n || cap < 0 || (cap > 0 && !out)) return fail(WSR_E_INVALID, "null argument");
  if (s->h != h) return fail(WSR_E_INVALID, "the doc set was made on another handle");
  *n = s->count;
  if (s->count > cap) return fail(WSR_E_LIMIT, "the set holds " + std::to_string(s->count) + " docs");
  if (s->count == 0) return WSR_OK;
  std::vector<uint32_t> bits(s->bits.size());
  try {
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipMemcpy(bits.data(), s->bits, s->bits.bytes(), hipMemcpyDeviceToHost));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  int64_t k = 0;
  for (size_t w = s->lo >> 5; w < bits.size() && k < s->count; ++w)
    for (uint32_t x = bits[w]; x; x &= x - 1u)
      out[k++] = static_cast<int32_t>(w * 32u + static_cast<uint32_t>(__builtin_ctz(x)));
  return WSR_OK;
}

extern "C" void wsr_docset_destroy(wsr_handle* h, wsr_docset* s) {
  if (!h || !s) return;
  (void)hipSetDevice(h->device);
  delete s;
}

extern "C" int wsr_count_bool_filtered(wsr_handle* h, const wsr_bool_query* q, int32_t nq,
                                       const wsr_docset* const* filters, int64_t* counts, int32_t item_blocks,
                                       wsr_or_stats* stats) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  if (item_blocks < 0 || item_blocks > kSegCost) return fail(WSR_E_INVALID, "item blocks must be 0..63");
  BoolPlan p;
  std::string why;
  const uint32_t target = item_blocks ? static_cast<uint32_t>(item_blocks) : h->args.seg_cap;
  int prc = plan_count(h->view(), q, nq, counts != nullptr, target, &p, &why);
  if (!prc) prc = check_filters(h, filters, nq, &why);
  if (prc) return fail(prc, why);
  if (!any_filter(filters, nq)) return wsr_count_bool_ex(h, q, nq, counts, item_blocks, stats);
  const std::vector<wsr_bool_query> live = without_empty_sets(q, nq, filters);
  if (!live.empty() && (prc = plan_count(h->view(), live.data(), nq, true, target, &p, &why)) != 0)
    return fail(prc, why);
  if (p.items.size() > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "over 2^32 boolean work items");
  if (p.items.empty()) {   // every query settled on the host
    for (int32_t i = 0; i < nq; ++i) counts[i] = 0;
    if (stats) *stats = wsr_or_stats{};
    return WSR_OK;
  }
  std::vector<const uint32_t*> table;
  apply_filters(&p, filters, &table);
  std::vector<int64_t> got(static_cast<size_t>(nq));
  wsr_or_stats sv{};
  const int rc = run_count(h, p, table, nq, got.data(), nullptr, 0, &sv);
  if (rc) return rc;
  std::copy(got.begin(), got.end(), counts);
  if (stats) *stats = sv;
  return WSR_OK;
}

extern "C" int wsr_search_bool_filtered(wsr_handle* h, const wsr_bool_query* q, int32_t nq,
                                        const wsr_docset* const* filters, int32_t hit_stride, wsr_hit* hits,
                                        int32_t* n_hits, int32_t item_blocks, wsr_or_stats* stats) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  if (item_blocks < 0 || item_blocks > kSegCost) return fail(WSR_E_INVALID, "item blocks must be 0..63");
  BoolPlan p;
  std::string why;
  const uint32_t target = item_blocks ? static_cast<uint32_t>(item_blocks) : h->args.seg_cap;
  int prc = plan_bool(h->view(), q, nq, hit_stride, hits && n_hits, target, &p, &why);
  if (!prc) prc = check_filters(h, filters, nq, &why);
  if (prc) return fail(prc, why);
  if (!any_filter(filters, nq)) return wsr_search_bool_ex(h, q, nq, hit_stride, hits, n_hits, item_blocks, stats);
  const std::vector<wsr_bool_query> live = without_empty_sets(q, nq, filters);
  if (!live.empty() && (prc = plan_bool(h->view(), live.data(), nq, hit_stride, true, target, &p, &why)) != 0)
    return fail(prc, why);
  const size_t n_q = p.qs.size(), n_items = p.items.size();
  if (n_items > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "over 2^32 boolean work items");
  const size_t n_rows = static_cast<size_t>(nq) * static_cast<size_t>(hit_stride > 0 ? hit_stride : 0);
  if (p.items.empty()) {   // every query settled on the host
    std::memset(hits, 0, sizeof(wsr_hit) * n_rows);
    std::memset(n_hits, 0, sizeof(int32_t) * static_cast<size_t>(nq));
    if (stats) *stats = wsr_or_stats{};
    return WSR_OK;
  }
  std::vector<const uint32_t*> table;
  apply_filters(&p, filters, &table);
  std::unique_ptr<BoolCtx> c = h->bool_pool.take();
  uint32_t ctr[kNumCounters];
  unsigned long long sv[kNumOrStats];
  try {
    HIP_OK(hipSetDevice(h->device));
    if (!c) {
      c.reset(new BoolCtx());
      c->st = gpu::make_stream();
      c->d_ctr.alloc(kNumCounters);
      c->d_stats.alloc(kNumOrStats);
    }
    if (n_q > c->d_qs.size()) gpu::alloc_group(n_q + n_q / 4, c->d_qs, c->d_roles);
    if (n_items > c->d_items.size()) gpu::alloc_group(n_items + n_items / 4 + 64, c->d_items, c->d_evcnt);
    c->d_filt.reserve(n_q, n_q + n_q / 4);
    c->d_events.reserve(p.ev_total, p.ev_total + p.ev_total / 4);
    c->d_hits.reserve(n_rows, n_rows + n_rows / 4);
    c->d_nhits.reserve(static_cast<size_t>(nq), static_cast<size_t>(nq) + static_cast<size_t>(nq) / 4);
    const hipStream_t st = c->st;
    HIP_OK(hipMemcpyAsync(c->d_qs, p.qs.data(), sizeof(OrQuery) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_roles, p.roles.data(), sizeof(BoolRoles) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_filt, table.data(), sizeof(const uint32_t*) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_items, p.items.data(), sizeof(OrItem) * n_items, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(c->d_ctr, 0, sizeof(uint32_t) * kNumCounters, st));
    HIP_OK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * kNumOrStats, st));
    // (the rows of the queries settled on the host, and every row past its n_hits)
    HIP_OK(hipMemsetAsync(c->d_hits, 0, sizeof(HitDev) * n_rows, st));
    HIP_OK(hipMemsetAsync(c->d_nhits, 0, sizeof(int32_t) * static_cast<size_t>(nq), st));
    HIP_OK(launch_bool_items_filtered(h->args, c->d_qs, c->d_roles, c->d_filt, c->d_items,
                                      static_cast<uint32_t>(n_items), p.nt_max, c->d_events, c->d_evcnt, c->d_ctr,
                                      c->d_stats, st));
    HIP_OK(launch_or_replay(c->d_qs, static_cast<uint32_t>(n_q), c->d_items, c->d_events, c->d_evcnt, c->d_hits,
                            hit_stride, c->d_nhits, p.narrow, p.wide, st));
    HIP_OK(hipMemcpyAsync(ctr, c->d_ctr, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(sv, c->d_stats, sizeof sv, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hits, c->d_hits, sizeof(HitDev) * n_rows, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(n_hits, c->d_nhits, sizeof(int32_t) * static_cast<size_t>(nq), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (const std::exception& e) {
    // (the context goes with what it holds, once its stream is idle)
    if (c && c->st) (void)hipStreamSynchronize(c->st);
    return fail(WSR_E_HIP, e.what());
  }
  h->bool_pool.give(std::move(c));
  if (ctr[kCtrError]) return fail(WSR_E_INTERNAL, "device reported error flags " + std::to_string(ctr[kCtrError]));
  if (stats) *stats = or_stats_of(sv);
  return WSR_OK;
}
