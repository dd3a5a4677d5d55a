// wsr_count_bool (include/wiser_hip.h): how many docs match each boolean
// query.  The host plans the call (bool_plan.cc, plan_count: wsr_search_bool's
// checks without k, the queries it can settle itself, the others' items); one
// launch of count_kernel writes every item's count and the host sums a
// query's items (bool_run.cc).
#include "bool_run.h"

using namespace wiser;

extern "C" int wsr_count_bool_ex(wsr_handle* h, const wsr_bool_query* q, int32_t nq, int64_t* counts,
                                 int32_t item_blocks, wsr_or_stats* stats) {
  BoolCall c;
  const int rc = plan_call(h, q, nq, nullptr, item_blocks, BoolMode::kCount, 0, counts != nullptr, stats, &c);
  if (rc || nq == 0) return rc;
  return run_bool(h, c, nq, count_out(counts), stats);
}

extern "C" int wsr_count_bool(wsr_handle* h, const wsr_bool_query* q, int32_t nq, int64_t* counts) {
  return wsr_count_bool_ex(h, q, nq, counts, 0, nullptr);
}
