// What the boolean entry points (bool_search.cc, count_bool.cc, docset.cc)
// share on the host: the front half of a call, up to a plan that can run, and
// the one function that runs such a plan on the device.
#pragma once

#include <vector>

#include "bool_plan.h"
#include "engine_impl.h"

namespace wiser {

enum class BoolMode { kSearch, kCount };   // plan_bool and bool_kernel / plan_count and count_kernel

// A planned call: the plan and, when some query has a doc set, table[i] = the
// bitmap of planned query i (NULL: none); empty when no query has one.
struct BoolCall {
  BoolPlan p;
  std::vector<const uint32_t*> table;
};

// Everything of a call before the device, in the order of its errors: h not
// NULL, item_blocks in 0..63, the plan of the queries as given (hit_stride: a
// search's; have_out: the output arrays are given), filters[0 .. nq) made on h
// (NULL entries and a NULL array are fine), the queries whose set is empty
// settled by a second plan, the 2^32 item limit, the items of filtered queries
// cut to their sets' ranges.  stats, when given, is zeroed once the checks of
// the queries and sets have passed.  WSR_OK, or the code with wsr_last_error
// set.  On WSR_OK the call is over if nq == 0 (nothing is planned and no
// output array need exist); else run_bool is due, and out->p.items is empty
// when every query is settled on the host.
int plan_call(wsr_handle* h, const wsr_bool_query* q, int32_t nq, const wsr_docset* const* filters,
              int32_t item_blocks, BoolMode mode, int32_t hit_stride, bool have_out, wsr_or_stats* stats,
              BoolCall* out);

// Where run_bool's answer goes.  A search: nq rows of hit_stride hits and
// n_hits[nq].  A count: counts[nq], written only once the call has succeeded,
// and, for wsr_docset_from_bool, the bitmap of out_words words that receives
// the matching docs' bits (zeroed here, on the call's stream; the call's
// table must then not be empty).
struct BoolOut {
  BoolMode mode;
  int32_t hit_stride;
  wsr_hit* hits;
  int32_t* n_hits;
  int64_t* counts;
  uint32_t* out_bits;
  size_t out_words;
};
inline BoolOut search_out(int32_t hit_stride, wsr_hit* hits, int32_t* n_hits) {
  return BoolOut{BoolMode::kSearch, hit_stride, hits, n_hits, nullptr, nullptr, 0};
}
inline BoolOut count_out(int64_t* counts, uint32_t* out_bits = nullptr, size_t out_words = 0) {
  return BoolOut{BoolMode::kCount, 0, nullptr, nullptr, counts, out_bits, out_words};
}

// Runs a planned call of nq > 0 queries.  A plan without items: hits and
// n_hits, or counts, are zeroed and nothing else happens (no context, no
// device work; out_bits is the caller's to settle).  Else, on the device in a
// context of h's pool: the tables up, one launch over the items (the filtered
// instance iff c.table is not empty), a search's replay, the answer down, one
// wait; stats, when given, receives the device's counters.  A HIP error is
// WSR_E_HIP and costs the context (destroyed once its stream is idle, not
// given back); a device error flag is WSR_E_INTERNAL.
int run_bool(wsr_handle* h, const BoolCall& c, int32_t nq, const BoolOut& out, wsr_or_stats* stats);

}  // namespace wiser
