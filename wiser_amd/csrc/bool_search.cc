// wsr_search_bool (include/wiser_hip.h): boolean queries of MUST, SHOULD and
// MUST_NOT terms.  The host plans the call (bool_plan.cc: checks, the queries
// it can settle itself, the others' items); one launch of bool_kernel writes
// the items' events and or_replay_kernel ranks each query's.
#include <cstring>

#include "bool_plan.h"
#include "engine_impl.h"

using namespace wiser;

static_assert(sizeof(wsr_hit) == sizeof(HitDev), "wsr_hit layout");

extern "C" int wsr_check_bool_query(wsr_handle* h, const wsr_bool_query* q) {
  if (!h || !q) return fail(WSR_E_INVALID, "null argument");
  std::string why;
  const int rc = check_bool_query(h->view(), *q, &why);
  return rc ? fail(rc, why) : WSR_OK;
}

extern "C" int wsr_search_bool_ex(wsr_handle* h, const wsr_bool_query* q, int32_t nq, int32_t hit_stride,
                                  wsr_hit* hits, int32_t* n_hits, int32_t item_blocks, wsr_or_stats* stats) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  if (item_blocks < 0 || item_blocks > kSegCost) return fail(WSR_E_INVALID, "item blocks must be 0..63");
  // (no handle lock: the image is read-only after wsr_open and each call works in a context of its own)
  BoolPlan p;
  std::string why;
  const uint32_t target = item_blocks ? static_cast<uint32_t>(item_blocks) : h->args.seg_cap;
  const int prc = plan_bool(h->view(), q, nq, hit_stride, hits && n_hits, target, &p, &why);
  if (prc) return fail(prc, why);
  if (stats) *stats = wsr_or_stats{};
  if (nq == 0) return WSR_OK;
  const size_t n_rows = static_cast<size_t>(nq) * static_cast<size_t>(hit_stride > 0 ? hit_stride : 0);
  if (p.items.empty()) {   // every query settled on the host
    std::memset(hits, 0, sizeof(wsr_hit) * n_rows);
    std::memset(n_hits, 0, sizeof(int32_t) * static_cast<size_t>(nq));
    return WSR_OK;
  }
  const size_t n_q = p.qs.size(), n_items = p.items.size();
  if (n_items > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "over 2^32 boolean work items");
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
    c->d_events.reserve(p.ev_total, p.ev_total + p.ev_total / 4);
    c->d_hits.reserve(n_rows, n_rows + n_rows / 4);
    c->d_nhits.reserve(static_cast<size_t>(nq), static_cast<size_t>(nq) + static_cast<size_t>(nq) / 4);
    const hipStream_t st = c->st;
    HIP_OK(hipMemcpyAsync(c->d_qs, p.qs.data(), sizeof(OrQuery) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_roles, p.roles.data(), sizeof(BoolRoles) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_items, p.items.data(), sizeof(OrItem) * n_items, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(c->d_ctr, 0, sizeof(uint32_t) * kNumCounters, st));
    HIP_OK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * kNumOrStats, st));
    // (the rows of the queries settled on the host, and every row past its n_hits)
    HIP_OK(hipMemsetAsync(c->d_hits, 0, sizeof(HitDev) * n_rows, st));
    HIP_OK(hipMemsetAsync(c->d_nhits, 0, sizeof(int32_t) * static_cast<size_t>(nq), st));
    HIP_OK(launch_bool_items(h->args, c->d_qs, c->d_roles, c->d_items, static_cast<uint32_t>(n_items), p.nt_max,
                             c->d_events, c->d_evcnt, c->d_ctr, c->d_stats, st));
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

extern "C" int wsr_search_bool(wsr_handle* h, const wsr_bool_query* q, int32_t nq, int32_t hit_stride,
                               wsr_hit* hits, int32_t* n_hits) {
  return wsr_search_bool_ex(h, q, nq, hit_stride, hits, n_hits, 0, nullptr);
}
