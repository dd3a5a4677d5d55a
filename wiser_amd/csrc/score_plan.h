// The host's plan of a wsr_score_docs call: a pure function of the queries,
// their candidate doc ids and the host copy of the image directory.  It
// validates the call, resolves each query's terms against the image, sorts
// each query's candidates by doc id (keeping each one's place in the caller's
// array) and cuts them into work items of at most kScoreLanes consecutive
// sorted candidates.  No HIP, no handle: tests/cpp/score_plan_check.cc runs it
// on the CPU.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wiser_hip.h"
#include "batch_plan.h"
#include "engine_types.h"

namespace wiser {

struct ScorePlan {
  std::vector<ScoreQuery> qs;      // one per query of the call
  std::vector<ScoreItem> items;
  // Per query i, at [doc_off[i], doc_off[i + 1]): its candidates in ascending
  // doc id, equal ids in the caller's order, and where each one came from
  // (docs[j] = the caller's docs[index[j]]): a permutation of [0, total).
  std::vector<uint32_t> docs, index;
};

// Candidates of one call at most (the index array holds 32-bit places).
constexpr int64_t kScoreMaxPairs = int64_t{1} << 31;

// Plans the call; n_docs: docs of the whole index (a shard image's too).
// *out is overwritten (its vectors keep their capacity).  Only the candidates
// inside the image's doc range, of queries with at least one term that has
// postings in the image, are put into items: every other row of the answer
// is {0.0, 0}.  WSR_OK, or the WSR_E_* code with its message in *err.
int plan_score_docs(const ImageView& v, int64_t n_docs, const wsr_query* q, int32_t nq, const int64_t* doc_off,
                    const int32_t* docs, ScorePlan* out, std::string* err);

}  // namespace wiser
