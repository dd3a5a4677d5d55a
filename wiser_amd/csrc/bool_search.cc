// wsr_search_bool (include/wiser_hip.h): boolean queries of MUST, SHOULD and
// MUST_NOT terms.  The host plans the call (bool_plan.cc: checks, the queries
// it can settle itself, the others' items); one launch of bool_kernel writes
// the items' events and or_replay_kernel ranks each query's (bool_run.cc).
#include "bool_run.h"

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
  BoolCall c;
  const int rc = plan_call(h, q, nq, nullptr, item_blocks, BoolMode::kSearch, hit_stride, hits && n_hits, stats, &c);
  if (rc || nq == 0) return rc;
  return run_bool(h, c, nq, search_out(hit_stride, hits, n_hits), stats);
}

extern "C" int wsr_search_bool(wsr_handle* h, const wsr_bool_query* q, int32_t nq, int32_t hit_stride,
                               wsr_hit* hits, int32_t* n_hits) {
  return wsr_search_bool_ex(h, q, nq, hit_stride, hits, n_hits, 0, nullptr);
}
