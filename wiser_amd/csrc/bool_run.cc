// The boolean calls' shared host code (bool_run.h): wsr_search_bool,
// wsr_count_bool, their filtered forms and wsr_docset_from_bool are plan_call,
// then run_bool in one of its two modes.
#include "bool_run.h"

#include <algorithm>
#include <cstring>

namespace wiser {
namespace {

// filters[0 .. nq) belong to h
int check_filters(const wsr_handle* h, const wsr_docset* const* filters, int32_t nq, std::string* err) {
  for (int32_t i = 0; i < nq; ++i)
    if (filters[i] && filters[i]->h != h) {
      *err = "query " + std::to_string(i) + ": the doc set was made on another handle";
      return WSR_E_INVALID;
    }
  return WSR_OK;
}

bool any_filter(const wsr_docset* const* filters, int32_t nq) {
  for (int32_t i = 0; i < nq; ++i)
    if (filters[i]) return true;
  return false;
}

// The call's queries with those whose set is empty turned into queries without
// terms, which the plan settles; empty when no set is empty.  (Only after the
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

}  // namespace

int plan_call(wsr_handle* h, const wsr_bool_query* q, int32_t nq, const wsr_docset* const* filters,
              int32_t item_blocks, BoolMode mode, int32_t hit_stride, bool have_out, wsr_or_stats* stats,
              BoolCall* out) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  if (item_blocks < 0 || item_blocks > kSegCost) return fail(WSR_E_INVALID, "item blocks must be 0..63");
  // (no handle lock: the image is read-only after wsr_open and each call works in a context of its own)
  const uint32_t target = item_blocks ? static_cast<uint32_t>(item_blocks) : h->args.seg_cap;
  BoolPlan& p = out->p;
  std::string why;
  const auto plan = [&](const wsr_bool_query* qs) {
    return mode == BoolMode::kSearch ? plan_bool(h->view(), qs, nq, hit_stride, have_out, target, &p, &why)
                                     : plan_count(h->view(), qs, nq, have_out, target, &p, &why);
  };
  int rc = plan(q);
  if (!rc && filters) rc = check_filters(h, filters, nq, &why);
  if (rc) return fail(rc, why);
  if (stats) *stats = wsr_or_stats{};
  const bool filtered = filters && any_filter(filters, nq);
  if (filtered) {
    const std::vector<wsr_bool_query> live = without_empty_sets(q, nq, filters);
    if (!live.empty() && (rc = plan(live.data())) != 0) return fail(rc, why);
  }
  if (p.items.size() > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "over 2^32 boolean work items");
  if (filtered) apply_filters(&p, filters, &out->table);
  return WSR_OK;
}

int run_bool(wsr_handle* h, const BoolCall& call, int32_t nq, const BoolOut& out, wsr_or_stats* stats) {
  const BoolPlan& p = call.p;
  const bool search = out.mode == BoolMode::kSearch, filtered = !call.table.empty();
  const size_t n_q = p.qs.size(), n_items = p.items.size(), n_out = static_cast<size_t>(nq);
  const size_t n_rows = search ? n_out * static_cast<size_t>(out.hit_stride > 0 ? out.hit_stride : 0) : 0;
  if (p.items.empty()) {   // every query settled on the host
    if (search) {
      std::memset(out.hits, 0, sizeof(wsr_hit) * n_rows);
      std::memset(out.n_hits, 0, sizeof(int32_t) * n_out);
    } else {
      std::fill(out.counts, out.counts + n_out, int64_t{0});
    }
    return WSR_OK;
  }
  std::unique_ptr<BoolCtx> c = h->bool_pool.take();
  uint32_t ctr[kNumCounters];
  unsigned long long sv[kNumOrStats];
  std::vector<uint32_t> icnt(search ? 0 : n_items);
  try {
    HIP_OK(hipSetDevice(h->device));
    if (!c) {
      c.reset(new BoolCtx());
      c->st = gpu::make_stream();
      c->d_ctr.alloc(kNumCounters);
      c->d_stats.alloc(kNumOrStats);
    }
    if (n_q > c->d_qs.size()) gpu::alloc_group(n_q + n_q / 4, c->d_qs, c->d_roles);
    if (n_items > c->d_items.size()) gpu::alloc_group(n_items + n_items / 4 + 64, c->d_items, c->d_item_n);
    if (filtered) c->d_filt.reserve(n_q, n_q + n_q / 4);
    if (search) {
      c->d_events.reserve(p.ev_total, p.ev_total + p.ev_total / 4);
      c->d_hits.reserve(n_rows, n_rows + n_rows / 4);
      c->d_nhits.reserve(n_out, n_out + n_out / 4);
    }
    const uint32_t* const* filt = filtered ? c->d_filt.get() : nullptr;
    const hipStream_t st = c->st;
    HIP_OK(hipMemcpyAsync(c->d_qs, p.qs.data(), sizeof(OrQuery) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_roles, p.roles.data(), sizeof(BoolRoles) * n_q, hipMemcpyHostToDevice, st));
    if (filtered)
      HIP_OK(hipMemcpyAsync(c->d_filt, call.table.data(), sizeof(const uint32_t*) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_items, p.items.data(), sizeof(OrItem) * n_items, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(c->d_ctr, 0, sizeof(uint32_t) * kNumCounters, st));
    HIP_OK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * kNumOrStats, st));
    if (search) {
      // (the rows of the queries settled on the host, and every row past its n_hits)
      HIP_OK(hipMemsetAsync(c->d_hits, 0, sizeof(HitDev) * n_rows, st));
      HIP_OK(hipMemsetAsync(c->d_nhits, 0, sizeof(int32_t) * n_out, st));
      HIP_OK(launch_bool_items(h->args, c->d_qs, c->d_roles, filt, c->d_items, static_cast<uint32_t>(n_items),
                               p.nt_max, c->d_events, c->d_item_n, c->d_ctr, c->d_stats, st));
      HIP_OK(launch_or_replay(c->d_qs, static_cast<uint32_t>(n_q), c->d_items, c->d_events, c->d_item_n, c->d_hits,
                              out.hit_stride, c->d_nhits, p.narrow, p.wide, st));
    } else {
      HIP_OK(hipMemsetAsync(c->d_item_n, 0, sizeof(uint32_t) * n_items, st));
      if (out.out_bits) HIP_OK(hipMemsetAsync(out.out_bits, 0, sizeof(uint32_t) * out.out_words, st));
      HIP_OK(launch_count_items(h->args, c->d_qs, c->d_roles, filt, c->d_items, static_cast<uint32_t>(n_items),
                                p.nt_max, c->d_item_n, out.out_bits, c->d_ctr, c->d_stats, st));
    }
    HIP_OK(hipMemcpyAsync(ctr, c->d_ctr, sizeof ctr, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(sv, c->d_stats, sizeof sv, hipMemcpyDeviceToHost, st));
    if (search) {
      HIP_OK(hipMemcpyAsync(out.hits, c->d_hits, sizeof(HitDev) * n_rows, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(out.n_hits, c->d_nhits, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, st));
    } else {
      HIP_OK(hipMemcpyAsync(icnt.data(), c->d_item_n, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
  } catch (const std::exception& e) {
    // (the context goes with what it holds, once its stream is idle)
    if (c && c->st) (void)hipStreamSynchronize(c->st);
    return fail(WSR_E_HIP, e.what());
  }
  h->bool_pool.give(std::move(c));
  if (ctr[kCtrError]) return fail(WSR_E_INTERNAL, "device reported error flags " + std::to_string(ctr[kCtrError]));
  if (!search) {
    for (int32_t i = 0; i < nq; ++i) out.counts[i] = 0;   // (the queries settled on the host)
    for (const OrQuery& oq : p.qs) {
      int64_t sum = 0;
      for (uint32_t j = 0; j < oq.n_items; ++j) sum += icnt[oq.item_base + j];
      out.counts[oq.q] = sum;
    }
  }
  if (stats) *stats = or_stats_of(sv);
  return WSR_OK;
}

}  // namespace wiser
