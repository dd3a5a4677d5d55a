// The host's plan of a batch upload (wsr_batch_upload): a pure function of the
// query array and the host copy of the image directory.  It validates the
// queries, fills the QueryIn array and the long queries' term table, cuts the
// disjunctive queries into items, sizes the event and item workspaces, and
// evaluates the device's class rule (plan_query_kernel, by the predicates of
// engine_types.h that both sides call) to size the persistent grids and to
// pick the kernel instances.  No HIP, no handle, no batch: tests/cpp/
// batch_plan_check.cc runs it on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wiser_hip.h"
#include "engine_types.h"

namespace wiser {

// What the plan reads of an open engine (read-only after wsr_open).
struct ImageView {
  const ListDev* lists = nullptr;         // host copy of the directory heads
  size_t n_lists = 0;
  const BlockDev* blocks = nullptr;       // host copy of the block directory
  size_t n_blocks = 0;
  const uint64_t* list_bytes = nullptr;   // docid+tf span bytes per list (n_lists)
  const uint64_t* pos_bytes = nullptr;    // position box bytes per list (null: positions off)
  float dense_ratio = 1.0f;
  uint32_t doc_lo = 0, doc_hi = 0;        // doc-id range of the image
  bool positions = false;
  // grid caps: lean workgroups (of kLeanWaves waves) of the conjunctive
  // instance, of its two-term instance and of the phrase instance; general workgroups
  int lean_wgs = 0, lean_wgs_two = 0, lean_wgs_ph = 0, gen_cap = 0;
};

// What a batch run needs to know of the uploaded queries.  (The defaults: a
// batch before its first upload.)
struct BatchClass {
  bool has_phrase = false;       // the uploaded queries include a phrase query
  bool gen_phrase = false;       // ... one of the general class (segment_kernel's phrase instance)
  bool has_conj_lean = true;     // the class rule found a conjunctive lean query
  bool has_gen = true;           // ... a general one
  bool has_wide = false;         // ... a query with k > kMaxK (wide_replay_kernel)
  bool two_conj = false;         // every conjunctive query: two terms (or empty), k <= kMaxK
  bool two_ph = false;           // every phrase query: k <= kMaxK (a lean one has two terms)
  bool one_conj = false;         // every conjunctive query: one term (or empty), and not two_conj
  bool has_or = false;           // the uploaded queries include an OR query (even an empty one)
  bool or_narrow = false, or_wide = false;   // some k <= kMaxK / > kMaxK among the OR table's
  int seg_grid = 0;              // general workgroups
  int lean_wgs = 0;              // the conjunctive lean instance's grid
  int lean_wgs_ph = 0;           // the phrase instance's (batches with phrase queries)
  int n_or = 0;                  // OR queries with at least one resolved term, k > 0 and an item
  uint32_t or_items = 0;
  int or_nt_max = 0;             // the most resolved terms of one of them
  uint64_t algo_static = 0;      // sum of list spans + k*12 over the uploaded queries
  // the tiny class (is_tiny_query), which only a plain run has (launches_of):
  // has_gen, seg_grid and the lean grids above count a tiny query in its other
  // class, as a shard step runs it
  int n_tiny = 0;                // tiny queries
  int seg_grid_rest = 0;         // general workgroups over those
};

struct UploadPlan {
  std::vector<QueryIn> in;       // one per query (an OR query: an empty row)
  std::vector<int32_t> ext;      // term lists of queries over kMaxTerms, after the QueryIn array
  std::vector<OrQuery> orq;      // the disjunctive queries' table, items and event total
  std::vector<OrItem> or_items;
  uint64_t or_ev = 0;
  uint64_t ev_need = 0, items_need = 0;   // event slots / work items of the conjunctive plan at most
  size_t q_bytes = 0;            // the QueryIn array and ext, as uploaded
  BatchClass cls;
};

// the list ids of a query in query order (list_ids, then more_ids)
std::vector<int32_t> query_terms(const wsr_query& q);

// wsr_check_query's rule: WSR_OK, or the code with its message in *err.
int check_query(const ImageView& v, const wsr_query& q, std::string* err);

// Plans the upload of q[0, nq) into a batch of hit stride `stride` and item
// length seg_cap; *out is overwritten (its vectors keep their capacity).
// WSR_OK, or the WSR_E_* code with its message in *err.
int plan_upload(const ImageView& v, const wsr_query* q, int32_t nq, int32_t stride, uint32_t seg_cap,
                UploadPlan* out, std::string* err);

// Which persistent kernels a run launches.  A batch with phrase queries
// launches the conjunctive lean kernel and the general one only when the class
// rule found such queries (an empty persistent launch waited for CU slots
// beside the others: 54 us on C5, profiles/r05p); the device plan flags
// kErrClass if a class without a launch holds items.  Shard steps launch
// everything (their owners read every query's emission), and a carried owner
// replay rides in the conjunctive launch, which runs then even with no
// conjunctive lean item of its own.
// A plain run (no shard step, no carried owner replay) has the tiny class
// (tiny_class): the device plan takes the tiny queries out of the other two
// classes, tiny_kernel is launched when the host counted any (tiny), and the
// general launch is sized by the general queries that are left (gen_grid
// workgroups; which batches launch it is the rule above, unchanged).  A plain
// run whose host count is zero keeps the class on, so that a tiny query the
// device plan finds all the same is flagged (kErrClass), not run elsewhere.
struct Launches {
  bool conj = true, gen = true;
  bool tiny = false;        // tiny_kernel is launched
  int gen_grid = 0;         // general workgroups of the launch (gen)
  bool tiny_class = false;  // the device plan classes tiny queries
};
constexpr Launches launches_of(const BatchClass& c, bool shard_step, bool carries_owner_replay) {
  const bool cls = !shard_step && !carries_owner_replay;
  return Launches{shard_step || carries_owner_replay || !c.has_phrase || c.has_conj_lean,
                  shard_step || !c.has_phrase || c.has_gen, cls && c.n_tiny > 0,
                  cls ? c.seg_grid_rest : c.seg_grid, cls};
}

}  // namespace wiser
