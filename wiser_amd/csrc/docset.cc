// Doc sets (include/wiser_hip.h, wsr_docset): a bitmap over the whole index's
// doc ids resident in HBM, built from ids on the host (wsr_docset_from_ids) or
// from a boolean query on the device (wsr_docset_from_bool: match_set_kernel),
// and the two calls that read one per query as a filter:
// wsr_search_bool_filtered (bool_filtered_kernel, then or_replay_kernel) and
// wsr_count_bool_filtered (count_filtered_kernel).  The plans are plan_bool's
// and plan_count's as they are; the sets go to the device as a table of
// bitmap pointers beside the BoolRoles table, one entry per planned query
// (bool_run.cc, which plans and runs all three).
#include <algorithm>
#include <vector>

#include "bool_run.h"

using namespace wiser;

namespace {

// words of a bitmap over n_docs docs, padded to whole windows (at least one)
size_t docset_words(int64_t n_docs) {
  const size_t windows = std::max<size_t>(1, (static_cast<size_t>(n_docs) + kOrWindow - 1) / kOrWindow);
  return windows * (kOrWindow / 32);
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
  BoolCall c;
  int rc = plan_call(h, q, 1, &within, item_blocks, BoolMode::kCount, 0, true, nullptr, &c);
  if (rc) return rc;
  const bool settled = c.p.items.empty();
  // (match_set_kernel always reads the table: one of NULLs without `within`)
  if (c.table.empty()) c.table.assign(c.p.qs.size(), nullptr);
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
    int64_t count = 0;
    rc = run_bool(h, c, 1, count_out(&count, s->bits, s->bits.size()), nullptr);
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
  BoolCall c;
  const int rc = plan_call(h, q, nq, filters, item_blocks, BoolMode::kCount, 0, counts != nullptr, stats, &c);
  if (rc || nq == 0) return rc;
  return run_bool(h, c, nq, count_out(counts), stats);
}

extern "C" int wsr_search_bool_filtered(wsr_handle* h, const wsr_bool_query* q, int32_t nq,
                                        const wsr_docset* const* filters, int32_t hit_stride, wsr_hit* hits,
                                        int32_t* n_hits, int32_t item_blocks, wsr_or_stats* stats) {
  BoolCall c;
  const int rc = plan_call(h, q, nq, filters, item_blocks, BoolMode::kSearch, hit_stride, hits && n_hits, stats, &c);
  if (rc || nq == 0) return rc;
  return run_bool(h, c, nq, search_out(hit_stride, hits, n_hits), stats);
}
