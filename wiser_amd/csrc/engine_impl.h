// What engine.cc (batches: upload, run, fetch, stats) and shard_exchange.cc
// (doc-range shard steps, communicators, deferred owner replays) share: the
// handle, the batch with its exchange state, and the C ABI's error slot.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wiser_hip.h"
#include "batch_plan.h"
#include "dev_mem.h"
#include "engine_types.h"
#include "index.h"
#include "kernels.h"
#include "shard_layout.h"
#include "snippet.h"

namespace wiser {
extern thread_local std::string g_err;   // wsr_last_error's (engine.cc)
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// tuning knobs read once per open (unset or unparsable: the default)
inline double env_number(const char* name, double dflt) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const double x = std::strtod(v, &end);
  return (end && *end == 0 && x >= 0) ? x : dflt;
}

// the traversal kernels' kNumOrStats counters as the C ABI's record
inline wsr_or_stats or_stats_of(const unsigned long long* v) {
  wsr_or_stats s{};
  s.items = v[kOrStatItems];
  s.windows = v[kOrStatWindows];
  s.windows_skipped = v[kOrStatSkipped];
  s.touched_docs = v[kOrStatTouched];
  s.events = v[kOrStatEvents];
  return s;
}
}  // namespace wiser

// A handle's reusable per-call contexts, one per concurrent caller.
template <class T>
class CtxPool {
 public:
  // an idle context, or null: the caller makes one
  std::unique_ptr<T> take() {
    std::lock_guard<std::mutex> g(mu_);
    if (idle_.empty()) return nullptr;
    std::unique_ptr<T> c = std::move(idle_.back());
    idle_.pop_back();
    return c;
  }
  // back after a call that went well (at most 8 are kept)
  void give(std::unique_ptr<T> c) {
    std::lock_guard<std::mutex> g(mu_);
    if (idle_.size() < 8) idle_.push_back(std::move(c));
  }

 private:
  std::mutex mu_;
  std::vector<std::unique_ptr<T>> idle_;
};

// What one wsr_score_docs call holds on the device (score_docs.cc): kept in a
// per-handle pool, one per concurrent caller, as wsr_search_batch's batches.
struct ScoreCtx {
  gpu::Stream st;
  gpu::DevBuf<wiser::ScoreQuery> d_qs;
  gpu::DevBuf<wiser::ScoreItem> d_items;
  gpu::DevBuf<uint32_t> d_docs, d_index;
  gpu::DevBuf<wiser::DocScore> d_out;
};

// What one boolean call holds on the device (bool_run.cc: wsr_search_bool,
// wsr_count_bool, their filtered forms and wsr_docset_from_bool): kept in a
// per-handle pool, one per concurrent caller, as the ScoreCtx.  The buffers a
// search alone needs are allocated by the first search the context serves.
struct BoolCtx {
  gpu::Stream st;
  gpu::DevBuf<wiser::OrQuery> d_qs;
  gpu::DevBuf<wiser::BoolRoles> d_roles;     // (sized together with d_qs)
  gpu::DevBuf<wiser::OrItem> d_items;
  // per item: its events (a search) or its matching docs (a count); sized together with d_items
  gpu::DevBuf<uint32_t> d_item_n;
  gpu::DevBuf<uint32_t> d_ctr;              // kNumCounters (the error flags)
  gpu::DevBuf<unsigned long long> d_stats;   // kNumOrStats
  gpu::DevBuf<const uint32_t*> d_filt;       // per query its doc set's bitmap (on first use)
  gpu::DevBuf<wiser::Event> d_events;        // search only, as d_hits and d_nhits (on first use)
  gpu::DevBuf<wiser::HitDev> d_hits;
  gpu::DevBuf<int32_t> d_nhits;
};

// A doc set (docset.cc): a bitmap over the doc ids of the whole index, bit
// d & 31 of word d >> 5 doc d, zero-padded to whole windows of kOrWindow docs
// (never empty: a NULL bitmap is "unfiltered" to the kernels).  Immutable once
// its creating call returns.
struct wsr_docset {
  wsr_handle* h = nullptr;        // the handle it was made on
  gpu::DevBuf<uint32_t> bits;
  int64_t count = 0;              // docs in the set
  uint32_t lo = 0, hi = 0;        // every doc of the set lies in [lo, hi)
};

struct wsr_handle {
  std::mutex mu;
  int device = 0;
  gpu::Stream stream;
  wiser::VacuumIndex idx;
  wiser::DocStore docs;                    // my.fdx / my.fdt when the index has them (snippets)
  std::unique_ptr<wiser::SkipRowCache> rows;   // decoded skip rows for the snippet stage
  std::mutex pool_mu;                   // wsr_search_batch's reusable batches
  std::vector<wsr_batch*> pool;
  wiser::IndexArgs args{};
  gpu::DevBuf<uint8_t> d_blob;
  gpu::DevBuf<wiser::ListDev> d_lists;
  gpu::DevBuf<wiser::BlockDev> d_blocks;
  gpu::DevBuf<uint32_t> d_last, d_meta;
  gpu::DevBuf<uint8_t> d_c4;
  gpu::DevBuf<double> d_cache;
  gpu::DevBuf<wiser::DenseEnt> d_dense;
  gpu::DevBuf<uint32_t> d_dense_rk;   // the bitmap entries' rank records
  gpu::DevBuf<uint32_t> d_bkt;        // offset buckets (entries and offset bytes)
  gpu::DevBuf<uint8_t> d_tf8, d_plen, d_impact;
  gpu::DevBuf<uint16_t> d_doc16;      // 16-bit doc ids of the eligible lists
  gpu::DevBuf<uint32_t> d_d16_blk;    //   and each list's run in them
  gpu::DevBuf<float> d_bmax;
  gpu::DevBuf<uint32_t> d_tails;
  gpu::DevBuf<uint8_t> d_pos_blob;    // positions (opened with wsr_open_opts::positions)
  gpu::DevBuf<wiser::PosDev> d_pos_lists;
  gpu::DevBuf<uint32_t> d_pos_pk, d_pos_tail, d_pos_start;
  gpu::DevBuf<uint8_t> d_blm;
  gpu::DevBuf<uint32_t> d_blm_hash;
  bool positions = false;
  uint32_t dense_lists = 0;
  wsr_image_info info{};            // HBM bytes of the image's buffers
  std::vector<wiser::ListDev> lists;       // host copy of the directory heads
  std::vector<uint64_t> list_bytes; // docid+tf span bytes per list in this image
  std::vector<uint64_t> pos_bytes;  // position box bytes per list (positions on)
  std::vector<wiser::BlockDev> blocks;     // host copy (debug decode)
  std::vector<uint32_t> meta;
  // host-exchange owner replays deferred into a later batch run's lean kernel
  // (wsr_shard_step_replay_deferred), oldest first
  std::mutex hdef_mu;
  std::deque<wsr_batch*> hdef_q;
  int grid = 0;        // general segment kernel: workgroups (one wave each)
  int lean_wgs = 0;    // lean kernel: workgroups of kLeanWaves waves
  int lean_wgs_ph = 0; // ... its phrase instance's
  int lean_wgs_two = 0; // ... its two-term instance's (one workgroup per CU past residency)
  int gen_cap = 0;     // general workgroups launched at most
  CtxPool<ScoreCtx> score_pool;         // wsr_score_docs' reusable contexts
  CtxPool<BoolCtx> bool_pool;           // the boolean calls' (bool_run.cc)
  // what the upload plan (batch_plan.h) reads of the handle
  wiser::ImageView view() const {
    wiser::ImageView v;
    v.lists = lists.data();
    v.n_lists = lists.size();
    v.blocks = blocks.data();
    v.n_blocks = blocks.size();
    v.list_bytes = list_bytes.data();
    v.pos_bytes = pos_bytes.empty() ? nullptr : pos_bytes.data();
    v.dense_ratio = args.dense_ratio;
    v.doc_lo = args.doc_lo;
    v.doc_hi = args.doc_hi;
    v.positions = positions;
    v.lean_wgs = lean_wgs;
    v.lean_wgs_two = lean_wgs_two;
    v.lean_wgs_ph = lean_wgs_ph;
    v.gen_cap = gen_cap;
    return v;
  }
};

// A batch's side of the doc-range shard exchange (shard_exchange.cc): its own
// exchange buffers (wsr_shard_step_emit / _replay; a step group uses the
// communicator's), the events that order an exchange against the batch's
// runs, and the protocol by which whoever needs the batch's results finds the
// owner replay of its last shard step.
struct ShardExchange {
  explicit ShardExchange(wsr_batch* b) : batch(b) {}
  wsr_batch* const batch;
  gpu::DevBuf<wiser::Event> send, recv;   // ShardLayout(qpr, slot).total(pairs) events each; on first use
  int pairs = 0;
  gpu::Event ev[2];   // emission done -> comm stream; exchange + owner replay done
  std::atomic<bool> pending{false};   // an owner replay (ev[1]) enqueued and not yet joined
  // owner replays asked of somebody else for this batch (the communicator's
  // worker thread, a later step group, another batch's run), and those
  // enqueued: ev[1] is only waited on once they agree (join)
  std::atomic<uint64_t> req{0};
  std::atomic<uint64_t> enq{0};
  // a step group's owner replay of this batch deferred (wsr_shard_steps) and
  // not yet enqueued: join has comm enqueue it first (atomic: a fetch on one
  // thread may race a step group on another; the communicator's pend_mu
  // orders what the two do with the group)
  std::atomic<wsr_comm*> comm{nullptr};
  bool fused = false;     // the last run emitted into exchange regions (fill counters after d_ctr)
  // a host-exchange owner replay of this batch waiting for another batch's
  // run to carry it (wsr_shard_step_replay_deferred); its regions are in
  // recv once ev[0] (recorded after their copy on st) has passed.  Set and
  // cleared under the handle's hdef_mu; whoever clears it counts the replay
  // in req first, so join waits for its enqueue
  std::atomic<wsr_handle*> hdef{nullptr};
  int32_t hdef_rank = 0;
  int world = 0, qpr = 0;   // the last emission's world and q_per_owner
  int64_t slot = 0;         //     and slot (the replay half must match them)
  wiser::ShardLayout layout() const { return wiser::ShardLayout(qpr, slot); }

  void request() { req.fetch_add(1, std::memory_order_acq_rel); }
  // A requested owner replay is enqueued: ok, ev[1] is recorded behind it;
  // not ok, it failed and there is nothing new to wait for (pending keeps what
  // an earlier replay left).  deferred: it was a step group's deferred replay,
  // the one comm stood for, so join has nothing left to flush.  The other
  // replays (the worker's of a group not deferred, a host exchange's) never
  // set comm, and clearing it for them could hide a communicator's deferred
  // replay of this batch from join, which would then wait for ever.
  void enqueued(bool ok, bool deferred) {
    if (ok) pending = true;
    if (deferred) comm.store(nullptr, std::memory_order_release);
    enq.fetch_add(1, std::memory_order_release);
  }
  // Is an owner replay of the batch outstanding?  First wait until every one
  // asked for is enqueued (those still deferred: enqueued now), so that ev[1]
  // is the record to wait on.
  bool join();
};

struct wsr_batch {
  int max_q = 0, stride = 0, nq = 0;
  gpu::DevBuf<uint8_t> d_qb;       // QueryIn[nq], then the term table of queries over kMaxTerms (bytes)
  wiser::QueryIn* d_q() const { return reinterpret_cast<wiser::QueryIn*>(d_qb.get()); }
  gpu::DevBuf<wiser::QueryPlan> d_plan;
  gpu::DevBuf<wiser::QueryDesc> d_desc;   // lean queries' work records
  gpu::DevBuf<wiser::PlanPart> d_part;    // plan pass 1 -> 2 partial sums, per kPlanThreads queries
  gpu::DevBuf<uint32_t> d_ctr;
  gpu::PinnedBuf<uint32_t> h_ctr;  // pinned host copy of the counters (fetch)
  gpu::DevBuf<wiser::Event> d_events;
  gpu::DevBuf<uint32_t> d_evcnt, d_itemq;   // per item: its events, its query (sized together with d_pub)
  gpu::DevBuf<wiser::HitDev> d_hits;
  gpu::DevBuf<int32_t> d_nhits;
  gpu::DevBuf<uint32_t> d_qdone;   // fused replay: completed items per query
  gpu::DevBuf<uint32_t> d_tinyq;   // the tiny list: max_q query indices, then each entry's match count
  gpu::DevBuf<uint64_t> d_pub;     // per item score floor
  gpu::DevBuf<uint32_t> d_stats;   // per general workgroup, then per lean wave: survivors, blocks
  gpu::DevBuf<uint32_t> d_ph;      // phrase scratch, gen_cap * kPhraseScratch (lazily)
  wiser::BatchClass cls;         // the uploaded queries' class flags, grids and OR counts (plan_upload)
  wiser::Launches launched;      // the persistent kernels of the last run (their stats rows are its own)
  uint32_t seg_cap = wiser::kSegCost;   // driver blocks per work item at most (wsr_batch_set_item_blocks)
  ShardExchange x{this};
  // disjunctive (OR) queries: their table, items and event slots, allocated
  // by the first upload that holds one (cls.n_or == 0: no extra launch)
  gpu::DevBuf<wiser::OrQuery> d_orq;
  gpu::DevBuf<wiser::OrItem> d_oritem;
  gpu::DevBuf<uint32_t> d_orevcnt;   // (sized together with d_oritem)
  gpu::DevBuf<wiser::Event> d_orev;
  gpu::DevBuf<unsigned long long> d_orstat;   // kNumOrStats counters of the last run
  gpu::Event ev[5];   // (timing events) [4]: lean kernel end
  // Each batch runs on its own streams, so consecutive batches overlap on the
  // device (one's plan and first items under the other's last items); the
  // general kernel goes to st2, forked from and joined back into st.  HIP maps
  // streams to its hardware queues (GPU_MAX_HW_QUEUES, 4) round-robin in
  // creation order, and kernels of one queue run in order: a batch creates
  // three streams (st_pad carries only the conjunctive lean kernel of batches
  // with phrase queries, beside the other two), so the lean kernels of consecutive
  // batches land on queues 3 apart, i.e. on all four in turn, instead of
  // alternating between two (with two streams per batch the C3 headline fell
  // from 21.7 to 18.9 M q/s and C2 from 35.0 to 29.6 M at unchanged per-batch
  // kernel times, profiles/r04a_bench.json).
  gpu::Stream st, st2, st_pad;   // (created in this order, wsr_batch_create; nothing relies on the order they go in)
  gpu::Event fork, join, join_ph;
  bool ran = false;
};

// One run of the batch (engine.cc).  se: a shard step, the run emits into
// those regions instead of replaying; oj: an earlier step group's owner
// replay for the lean kernel's tail (its exchange is done).
int batch_run(wsr_handle* h, wsr_batch* b, const wiser::EmitView* se = nullptr, const wiser::OwnerJob* oj = nullptr);
// The host-deferred owner replays a run carries (shard_exchange.cc): the
// oldest one that a run of b can take (not b's own), off the queue and
// counted in its req, its job in *oj; and a taken one on pb's own stream
// after all (whether ev[1] is recorded behind it).
wsr_batch* take_host_replay(wsr_handle* h, const wsr_batch* b, wiser::OwnerJob* oj);
bool host_replay_enqueue(wsr_batch* pb, wsr_handle* h);
