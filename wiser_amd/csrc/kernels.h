// Launch interface of kernels.hip (host side).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine_types.h"

namespace wiser {

// Kernel view of one HBM index image (a whole index or one doc-range shard).
struct IndexArgs {
  const uint8_t* blob;      // [docid | tf] spans of every list, byte-exact from my.vacuum
  const ListDev* lists;
  const BlockDev* blocks;
  const uint32_t* blk_last; // dense copy of BlockDev::last for the block searches
  const uint32_t* blk_meta; // docid pack bits | tf pack bits << 8 (0 = VInts blob)
  const uint8_t* c4;        // 1-byte lossy doc length per doc id
  const double* cache;      // Bm25Similarity cache_[256]
  uint32_t n_c4;
  uint32_t n_lists;
  uint32_t doc_lo, doc_hi;  // doc-id range of this image (shard)
  double avg;               // average doc length stored in my.doc_length
  const DenseEnt* dense;    // rank bitmaps of the dense lists (ListDev::bm)
  const uint32_t* dense_rk; // their rank records (same index, kRankWords u32 each)
  const uint2* bkt;         // offset buckets of the sparser dense lists (ListDev::bm with a shift)
  const uint8_t* tf8;       // their 1-byte tfs (ListDev::tf8)
  uint32_t dense_span;      // bitmaps cover doc ids [doc_lo, doc_lo + dense_span)
  float dense_ratio;        // probe list B by bitmap when nblk(B) >= dense_ratio * nblk(driver)
  uint32_t seg_cap;         // driver blocks per work item at most (kSegCost; the batch's own, see
                            // wsr_batch_set_item_blocks: a latency-bound caller takes shorter items)
  const uint8_t* plen;      // doc-length code of each posting, 128 per block (HostImage::plen)
  const float* bmax;        // per block: its largest TfNormLossy, f32 rounded up (HostImage::bmax)
  const uint8_t* impact;    // impact byte of each posting, 128 per block as plen (HostImage::impact)
  const uint16_t* doc16;    // doc id - BlockDev::prev of each posting of the eligible lists, 128 per
                            // block (HostImage::doc16)
  const uint32_t* d16_blk;  // per list: the first block of its run in doc16, kNoDoc16 when it has
                            // none (null: the array was not built)
  float norm_min;           // the smallest doc-length norm of the image's postings, f32 rounded down
                            // (HostImage::norm_min): the lean pipeline bounds the other terms there
  const uint32_t* tails;    // decoded VInts last blocks (ListDev::tail)
  // positions (phrase queries; null unless the engine was opened with them)
  const uint8_t* pos_blob;  // every list's position cozy box, byte-exact from my.vacuum
  const PosDev* pos_lists;  // indexed by list id
  const uint2* pos_pk;      // per full pack: byte offset from PosDev::base, bit width
  const uint32_t* pos_tail; // decoded VInts remainders
  const uint2* pos_start;   // per posting (128 slots per image block): the bag's start entry,
                            // the pack it starts in (offset << 6 | width; 0: read pos_pk)
  // phrase bloom filters (null / 0 unless a bloom index was opened with
  // positions and bloom_factor > 0): per posting slot two 16-byte bit arrays
  // (prior, next), per list its term's two hashes; bloom_factor as
  // CheckBloomWithEnableFactor's (query_processing.h:796-807)
  const uint4* blm;
  const uint2* blm_hash;
  uint32_t blm_bits, blm_hashes, bloom_factor;
};

// counters[] (zeroed before every batch): 0 total items, 2 event capacity used,
// 4 error flags, 6 end of the lean items, 8 end of the conjunctive lean items,
// 10 entries of the batch's tiny list
// (items [0, lean conj) run in lean_kernel's conjunctive instance, [lean
// conj, lean) -- the lean phrase queries' -- in its phrase instance, the rest
// in segment_kernel); each work queue has one head per XCD-sized shard, each
// on its own 64-byte line (kCtrHead0 + 16*s lean conjunctive, kCtrPHead0 +
// 16*s lean phrase, kCtrGHead0 + 16*s general), so the dequeues of the
// persistent workers do not serialise on a single line.  A tiny query has no
// item: plan_query_kernel appends it to the batch's tiny list (kCtrTiny
// entries, in no particular order), which tiny_kernel's plain grid runs.
enum { kCtrItems = 0, kCtrEvCap = 2, kCtrError = 4, kCtrLean = 6, kCtrLeanConj = 8, kCtrTiny = 10, kCtrHead0 = 16,
       kQueueShards = 8,
       kCtrPHead0 = kCtrHead0 + 16 * kQueueShards,
       kCtrGHead0 = kCtrPHead0 + 16 * kQueueShards,
       kNumCounters = kCtrGHead0 + 16 * kQueueShards };
// QueryPlan::driver = driver slot | cost bucket << kPlanBucketShift | kPlanLean
// (| kPlanPhrase: a lean phrase query, the phrase instance's items), or
// kPlanTiny alone: a tiny query (is_tiny_query, engine_types.h)
constexpr uint32_t kPlanSlotMask = 0x7FFu;   // (kMaxQueryTerms <= 2048)
constexpr int kPlanBucketShift = 12;
constexpr uint32_t kPlanLean = 1u << 16;
constexpr uint32_t kPlanPhrase = 1u << 17;
constexpr uint32_t kPlanTiny = 1u << 18;
static_assert(kMaxQueryTerms <= static_cast<int>(kPlanSlotMask) + 1, "driver slot field");
// per-workgroup statistics written by the segment kernels (no atomics):
// stats[wg * kStatStride + {0 survivors, 1 driver blocks, 2 other blocks}]
// (a lean wave's row: 2 = of its driver blocks, those with postings in range whose D stage kept none, lean_segment)
constexpr int kStatStride = 4;
enum { kErrLimit = 1, kErrCapacity = 2, kErrExchange = 4, kErrClass = 8 };
constexpr int kMaxOwners = 1024;   // doc-range shards (ranks) of one exchange

// (kLeanWaves, kSegCost and kSingleWindows: engine_types.h, with the class rule)
// Driver blocks per item of a phrase query at most: a batch's phrase items
// are its tail when they are few (the realistic mix in log order: 15.4 -> 16.5
// M q/s at 32 against 63, C5 unchanged; 16: 16.0 / 8.5 M, round 5).  Since the
// batch former puts phrases in batches of their own (round 6), 48: C5 15.3 ->
// 16.1 M, the class-ordered mix 27.6 -> 27.2 M (63: 16.1 / 27.2 M;
// profiles/r06/phrase_cap_ab/).
constexpr uint32_t kPhraseSegCap = 48;
// item cost classes for the longest-first queue order (QueryPlan::driver >> kPlanBucketShift);
// kItemFixedCost = an item's setup (dequeue, directory loads), in block decodes
// item cost buckets: log2(cost) < 3, 3, 4, >= 5, and (the heaviest) the items
// of a query of at least kHeavyQueryItems items
constexpr int kCostBuckets = 5;
// A query of this many items or more is queued before every other item of
// its class: its replay, the batch's longest chain of heap insertions, then
// starts while the lighter items still run, instead of ending the batch.
constexpr uint32_t kHeavyQueryItems = 4;
constexpr float kItemFixedCost = 4.0f;

// Replay fused into the segment kernel: the workgroup that completes a
// query's last item replays it (q_done: per-query completed items, zeroed by
// the plan kernel).  q_done == nullptr: no fusion (separate replay launch, or
// doc-range shard mode where events are exchanged first).
//
// Fused shard emission (wsr_shard_step, x_send != nullptr): the worker that
// completes a query's last item reduces the query's events to those of a heap
// run from empty over this shard (EventFilter; every survivor for k > kMaxK),
// appends them to the owner's slot of the send buffer at an offset taken from
// the owner's fill counter, and records {count, offset} for the query
// (count -1 and kErrExchange when the slot is full).  No reduce, scan or pack
// launch is left between the segment kernels and the exchange.
// A deferred owner replay (wsr_shard_steps): after their own items, the waves
// of a lean kernel replay owned queries of an earlier step group's exchange --
// owner_replay_meta_kernel's work without its launch (OwnerJob, engine_types.h;
// nq 0: none).  Only batches without wide queries are deferred.
struct FusedReplay {
  uint32_t* q_done;
  HitDev* hits;
  int hit_stride;
  int32_t* n_hits;
  Event* x_send;        // owner o's slot at x_send + o * x_stride (x_slot events)
  int32_t* x_meta;      // {count, offset in the owner's slot} of query i of owner o at
                        //   x_meta + o * x_meta_stride + 2 * i
  uint32_t* x_fill;     // per owner: events appended (zeroed before the batch)
  uint32_t* x_err;      // error flags word
  uint64_t x_slot;      // slot capacity (events)
  uint64_t x_stride;    // events between owners' slots
  uint64_t x_meta_stride;   // int32 between owners' meta blocks
  int32_t x_qpr;        // queries per owner
  OwnerJob oj;          // (lean kernel only)
  __device__ int32_t* meta_of(uint32_t q) const {
    const uint32_t o = q / static_cast<uint32_t>(x_qpr);
    return x_meta + o * x_meta_stride + 2ull * (q - o * static_cast<uint32_t>(x_qpr));
  }
};

// Plan pass 1 -> pass 2: per plan workgroup (kPlanThreads queries), its items
// per item key (class, cost bucket) and its event capacity.
constexpr int kPlanThreads = 256;
constexpr int kPlanKeys = 3 * kCostBuckets;   // classes: lean conjunctive, lean phrase, general
struct PlanPart {
  uint32_t items[kPlanKeys];
  uint64_t cap;
};

// phrase scratch words per general workgroup / lean wave (null when the batch
// has no phrase query)
constexpr int kPhraseScratch = kMaxPhraseTerms * 256;

// plan queries (2 launches); part: per plan workgroup of kPlanThreads queries;
// tiny_grid: the tiny queries the host counted, for which it launches
// tiny_kernel (< 0: the run has no tiny class, its queries stay lean or
// general); tiny_q: the batch's tiny list, which pass 1 fills (the queries'
// indices, at least nq words)
hipError_t launch_plan(const IndexArgs& ix, const QueryIn* q, int nq, QueryPlan* plan,
                       uint32_t* counters, uint64_t ev_capacity, uint32_t item_capacity,
                       int lean_grid, int lean_grid_ph, int seg_grid, int tiny_grid, uint32_t* tiny_q,
                       const FusedReplay& fr, uint32_t* item_q, uint64_t* pub, QueryDesc* desc, PlanPart* part,
                       hipStream_t st);
// The tiny queries of a plain run (is_tiny_query), one wave each, n_tiny waves
// at least: both decoded tails met in the wave, every match scored and handed
// in doc order to the restated heap; hits and n_hits are written here.
// tiny_q: cap query indices (the plan's list), then cap words that receive
// each entry's match count.
hipError_t launch_tiny(const IndexArgs& ix, const QueryIn* q, const uint32_t* counters, uint32_t* tiny_q,
                       uint32_t cap, int n_tiny, HitDev* hits, int hit_stride, int32_t* n_hits, hipStream_t st);
hipError_t launch_segments(const IndexArgs& ix, const QueryIn* q, const QueryPlan* plan, int nq,
                           uint32_t* counters, Event* events, uint32_t* ev_cnt, uint32_t* stats,
                           int grid, const FusedReplay& fr, const uint32_t* item_q,
                           uint64_t* pub, uint32_t* ph, hipStream_t st);

// lean_grid workgroups of kLeanWaves waves; stats of wave w at stats[w * kStatStride];
// phrase: the lean phrase queries' items (the phrase instance; their lean
// ones have two terms), else the conjunctive lean items;
// two: every query of those items has two terms and k <= kMaxK;
// one (conjunctive only): every query of those items has one term
hipError_t launch_lean(const IndexArgs& ix, const QueryIn* q, const QueryPlan* plan, int nq,
                       uint32_t* counters, Event* events, uint32_t* ev_cnt, uint32_t* stats,
                       int lean_wgs, const FusedReplay& fr, const uint32_t* item_q,
                       uint64_t* pub, const QueryDesc* desc, bool phrase, bool two, bool one,
                       hipStream_t st);
int lean_kernel_occupancy(bool phrase);   // workgroups per CU
// queries with k > kMaxK (their segments emitted every survivor): heap in LDS
hipError_t launch_wide_replay(const QueryIn* q, const QueryPlan* plan, int nq, const Event* events,
                              const uint32_t* ev_cnt, HitDev* hits, int hit_stride, int32_t* n_hits,
                              hipStream_t st);
hipError_t launch_decode_probe(const uint8_t* p, uint32_t bits, uint32_t cnt, bool delta,
                               uint32_t seed, uint32_t* out, hipStream_t st);
// owner side of the fused exchange, as a launch of its own (any_wide: the
// LDS-heap instance too, for the job's queries with k > kMaxK)
hipError_t launch_owner_replay(const OwnerJob& oj, bool any_wide, hipStream_t st);
// resident 64-thread segment workgroups per CU
int segment_kernel_occupancy();

// Disjunctive (OR) queries: one wave per item accumulates every term's BM25
// into an LDS window of kOrWindow docs, term by term in query order, and
// emits the touched docs in doc order through the item's running top-k
// (every touched doc for k > kMaxK); ev_cnt[i] = events of item i; stats:
// kNumOrStats u64 (zeroed by the caller).  nt_max: the most resolved terms of
// a query of the table (sizes the decoded-block cache in LDS).
hipError_t launch_or_items(const IndexArgs& ix, const OrQuery* oq, const OrItem* items, uint32_t n_items,
                           int nt_max, Event* events, uint32_t* ev_cnt, uint32_t* counters,
                           unsigned long long* stats, hipStream_t st);
// one wave per OR query: its items' events, in doc order, through the
// restated heap (narrow: k <= kMaxK in the wave's lanes; wide: in LDS)
hipError_t launch_or_replay(const OrQuery* oq, uint32_t n_or, const OrItem* items, const Event* events,
                            const uint32_t* ev_cnt, HitDev* hits, int hit_stride, int32_t* n_hits,
                            bool narrow, bool wide, hipStream_t st);

// Boolean queries (wsr_search_bool): or_kernel's traversal body (window_item),
// instantiated with, per doc of the window, the set of slots that held it; a
// touched doc reaches the item's running top-k (or its event slot, k > kMaxK) only if it satisfies roles[q]
// (engine_types.h, BoolRoles).  oq[i] and roles[i] describe one query; the
// events are replayed by launch_or_replay over the same oq table.  filt: NULL
// (bool_kernel), or the call's doc-set table (bool_filtered_kernel): filt[i]
// is the set of query oq[i], NULL for none -- a bitmap over the whole index's
// docs, bit d & 31 of word d >> 5 doc d, zero-padded to whole windows of
// kOrWindow docs; a doc matches only if its bit is set, and a window without
// a set doc is not run.
hipError_t launch_bool_items(const IndexArgs& ix, const OrQuery* oq, const BoolRoles* roles,
                             const uint32_t* const* filt, const OrItem* items, uint32_t n_items, int nt_max,
                             Event* events, uint32_t* ev_cnt, uint32_t* counters, unsigned long long* stats,
                             hipStream_t st);

// Exact match counts (wsr_count_bool): one wave per item of plan_count's
// tables (oq[i], roles[i] and filt as for launch_bool_items; k, ubsum and the
// items' event slots are not read).  item_count[i] = matching docs of item
// i's range; every item of the launch is written.  counters: the error
// flags; stats: kNumOrStats u64 (zeroed by the caller), of which items,
// windows and touched docs are counted.  nt_max sizes the decoded-block cache
// in LDS (128 doc ids per slot).  out_bits not NULL: match_set_kernel, which
// also ORs every matching doc's bit into that zeroed bitmap (filt is then a
// table, of NULLs if need be, and describes one query); else filt not NULL:
// count_filtered_kernel; else count_kernel.
hipError_t launch_count_items(const IndexArgs& ix, const OrQuery* oq, const BoolRoles* roles,
                              const uint32_t* const* filt, const OrItem* items, uint32_t n_items, int nt_max,
                              uint32_t* item_count, uint32_t* out_bits, uint32_t* counters,
                              unsigned long long* stats, hipStream_t st);

// Given (query, doc) pairs (wsr_score_docs): one wave per item of at most
// kScoreLanes candidates, sorted by doc id at docs[first ..]; the answer of
// candidate j goes to out[index[j]].  Rows no item covers are left as they are
// (the caller zeroes out).
hipError_t launch_score_docs(const IndexArgs& ix, const ScoreQuery* qs, const ScoreItem* items, uint32_t n_items,
                             const uint32_t* docs, const uint32_t* index, DocScore* out, hipStream_t st);

}  // namespace wiser
