// The host's plan of a wsr_search_bool call: a pure function of the queries
// and the host copy of the image directory.  It validates the call, resolves
// each query's term slots against the image, settles on the host the queries
// that cannot match anything, and cuts the others into work items with
// plan_or_query (or_plan.h).  No HIP, no handle: tests/cpp/bool_plan_check.cc
// runs it on the CPU.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wiser_hip.h"
#include "batch_plan.h"
#include "engine_types.h"

namespace wiser {

struct BoolPlan {
  // One entry per query that reaches the device, qs[i] and roles[i] together
  // (engine_types.h, BoolRoles).  A SHOULD or MUST_NOT slot whose term is
  // missing or has no block in the image is dropped: the masks are over the
  // kept slots, in query order.  Every other query is settled here and has no
  // entry and no item: k <= 0, no terms, a MUST term missing or without a
  // block in the image, fewer kept SHOULD slots than need_should (which
  // covers a query of MUST_NOT terms only).
  std::vector<OrQuery> qs;
  std::vector<BoolRoles> roles;
  std::vector<OrItem> items;
  uint64_t ev_total = 0;     // event slots of all items
  int nt_max = 0;            // the most kept slots of one query
  bool narrow = false, wide = false;   // some k <= kMaxK / > kMaxK among qs
};

// wsr_check_bool_query's rule: WSR_OK, or the code with its message in *err.
int check_bool_query(const ImageView& v, const wsr_bool_query& q, std::string* err);

// Plans the call; have_out: hits and n_hits are both given; target: blocks per
// item over all of a query's lists (IndexArgs::seg_cap).  *out is overwritten
// (its vectors keep their capacity).  WSR_OK, or the WSR_E_* code with its
// message in *err.
//
// MaxScore sums (OrQuery::ubsum) run over the MUST and SHOULD slots only; a
// MUST_NOT slot's is 0.0 and the kernel never counts it as essential.  With a
// MUST term a matching doc is a posting of the lead list: an item without a
// lead block is dropped and every other item's event slot is capped by 128 x
// the lead blocks that overlap its range.
int plan_bool(const ImageView& v, const wsr_bool_query* q, int32_t nq, int32_t stride, bool have_out,
              uint32_t target, BoolPlan* out, std::string* err);

// The plan of a wsr_count_bool call: plan_bool's checks, kept slots, roles,
// lead and items (the same doc ranges, the items without a lead block
// dropped), without k: k is neither checked nor read (no "k <= 0 is settled",
// OrQuery::k is 0, narrow and wide stay false) and no event slot is sized
// (every ev_cap and ev_base, and ev_total, are 0).  have_out: counts is given.
int plan_count(const ImageView& v, const wsr_bool_query* q, int32_t nq, bool have_out, uint32_t target,
               BoolPlan* out, std::string* err);

}  // namespace wiser
