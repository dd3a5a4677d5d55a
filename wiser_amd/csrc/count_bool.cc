// wsr_count_bool (include/wiser_hip.h): how many docs match each boolean
// query.  The host plans the call (bool_plan.cc, plan_count: wsr_search_bool's
// checks without k, the queries it can settle itself, the others' items); one
// launch of count_kernel writes every item's count and the host sums a
// query's items.
#include <vector>

#include "bool_plan.h"
#include "engine_impl.h"

using namespace wiser;

extern "C" int wsr_count_bool_ex(wsr_handle* h, const wsr_bool_query* q, int32_t nq, int64_t* counts,
                                 int32_t item_blocks, wsr_or_stats* stats) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  if (item_blocks < 0 || item_blocks > kSegCost) return fail(WSR_E_INVALID, "item blocks must be 0..63");
  // (no handle lock: the image is read-only after wsr_open and each call works in a context of its own)
  BoolPlan p;
  std::string why;
  const uint32_t target = item_blocks ? static_cast<uint32_t>(item_blocks) : h->args.seg_cap;
  const int prc = plan_count(h->view(), q, nq, counts != nullptr, target, &p, &why);
  if (prc) return fail(prc, why);
  if (nq == 0) {
    if (stats) *stats = wsr_or_stats{};
    return WSR_OK;
  }
  const size_t n_q = p.qs.size(), n_items = p.items.size();
  if (n_items > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "over 2^32 boolean work items");
  if (p.items.empty()) {   // every query settled on the host
    for (int32_t i = 0; i < nq; ++i) counts[i] = 0;
    if (stats) *stats = wsr_or_stats{};
    return WSR_OK;
  }
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
    const hipStream_t st = c->st;
    HIP_OK(hipMemcpyAsync(c->d_qs, p.qs.data(), sizeof(OrQuery) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_roles, p.roles.data(), sizeof(BoolRoles) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_items, p.items.data(), sizeof(OrItem) * n_items, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(c->d_ctr, 0, sizeof(uint32_t) * kNumCounters, st));
    HIP_OK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * kNumOrStats, st));
    HIP_OK(hipMemsetAsync(c->d_icnt, 0, sizeof(uint32_t) * n_items, st));
    HIP_OK(launch_count_items(h->args, c->d_qs, c->d_roles, c->d_items, static_cast<uint32_t>(n_items), p.nt_max,
                              c->d_icnt, c->d_ctr, c->d_stats, st));
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

extern "C" int wsr_count_bool(wsr_handle* h, const wsr_bool_query* q, int32_t nq, int64_t* counts) {
  return wsr_count_bool_ex(h, q, nq, counts, 0, nullptr);
}
