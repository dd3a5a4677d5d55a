// Plain structs shared by the host planner and the HIP kernels.  All of them
// live in HBM; sizes are fixed so the host and device agree byte for byte.
#pragma once

#include <cstdint>

namespace wiser {

constexpr int kMaxTerms = 16;        // terms held inline in a QueryIn (and the plan's one-round loads)
constexpr int kMaxQueryTerms = 1024; // terms per conjunctive query (past kMaxTerms: QueryIn::ext)
constexpr int kMaxPhraseTerms = 8;   // terms per phrase query (the reference's cap, query_processing.h:695)
constexpr int kMaxK = 64;            // n_results of the wave top-k: running top-k and heap in one wave's lanes
constexpr int kMaxKWide = 1024;      // n_results per query; k > kMaxK: every survivor is an event and the
                                     // replay keeps the heap in LDS (wide_replay_kernel)

// One posting list in the HBM image.
struct ListDev {
  uint64_t base;      // byte offset of the list's docid span in the blob
  uint32_t blk0;      // first entry in the block directory
  uint32_t nblk;      // blocks of this list in the image
  uint32_t df;        // GLOBAL document frequency (drives idf and planning)
  uint32_t tail_cnt;  // postings in the image's last block (128 unless a VInts tail)
  double idf;         // calc_es_idf(N, df) computed on the host with libm log
  uint64_t bm;        // first DenseEnt of the list's doc bitmap, kNoDense when it has none
  uint64_t tf8;       // byte offset of the list's 1-byte tf array (posting order)
  uint64_t tail;      // its last block decoded (tail_cnt doc ids, then tail_cnt tfs) in the
                      // image's tails array when that block is a VInts blob, else kNoTail
  uint32_t last;      // last doc id of its last block in the image (= blk_last of that block)
  uint32_t tfmax;     // an upper bound of its tfs in the image: exact for dense lists (their tfs
                      // are decoded at load), else the largest pack width's maximum (~0u: unknown)
};
static_assert(sizeof(ListDev) == 64, "ListDev layout");
constexpr uint64_t kNoTail = ~0ull;

constexpr uint64_t kNoDense = ~0ull;
constexpr uint8_t kTf8Escape = 255;   // tf >= 255: read the tf blob instead

// Impact byte of a posting (HostImage::impact): q with q * kImpactScale >=
// tf / (tf + cache_[c4]), the tf part of its BM25 term without the 2.2 * idf
// factor.  The scale is the f32 just above 1/255, so 255 dequantises to >= 1,
// above every exact value (norms are > 0), and the lean pipeline bounds a
// driver posting's own term by b_id * kImpactScale * q with one byte-to-float
// conversion and one fma.
constexpr float kImpactScale = 0x1.010102p-8f;
inline double impact_value(uint32_t q) { return static_cast<double>(static_cast<float>(q) * kImpactScale); }
// the byte the loader stores for a posting of term frequency tf in a doc of
// length norm nrm (the real tf, also where tf8 holds the escape)
inline uint8_t impact_byte(uint32_t tf, double nrm) {
  const double f = static_cast<double>(static_cast<int32_t>(tf));
  const double x = f / (f + nrm);
  if (!(x > 0.0)) return 0;
  if (!(x < 1.0)) return 255;
  uint32_t q = static_cast<uint32_t>(x * 255.0);   // floor; the loop rounds up
  while (q < 255 && impact_value(q) < x) ++q;
  return static_cast<uint8_t>(q);
}

// 16-bit doc ids of a driver (HostImage::doc16): slot p of block b holds
// doc(b, p) - BlockDev::prev(b), so the lean pipeline reads a posting's doc id
// as one add instead of unpacking and prefix-summing the block's deltas.  A
// block is eligible when it is a full pack block whose last - prev fits 16
// bits; a list when every pack block of it in the image is (at least one; its
// VInts tail block is not counted: the kernels read the decoded tail).  Only
// eligible lists have a run in the array, one entry per block of the list in
// the image, the tail block's zero (HostImage::d16_blk).
constexpr uint32_t kDoc16Span = 65535;
constexpr uint32_t kNoDoc16 = ~0u;
inline bool doc16_block_ok(bool full_pack, uint32_t prev, uint32_t last) {
  return full_pack && last >= prev && last - prev <= kDoc16Span;
}

// A list's probe structure (ListDev::bm, QueryDesc::o_bm): bits 0-55 its
// first entry, bits 56-63 the bucket shift c (0: a rank bitmap of DenseEnt).
//
// Offset buckets (c = 3..8) are for lists of density below 1/kBucketDensity
// in the image's doc range, where a bitmap costs a 128-byte line per 1,024
// docs probed whatever the list holds: a driver a few hundred docs apart
// fetches nearly every mask line of the range, ~8x the list's compressed
// bytes at 1 % density (scripts/traffic_model.py).  The range is cut into
// buckets of 2^c docs, c chosen so that a bucket holds 1-2 postings on
// average (below 2.5 % density that is >= 64 docs: an entry line covers at
// least as many docs as a mask line); per bucket
// one 8-byte BucketEnt {rank << 9 | count, the in-bucket
// offsets (doc - bucket start) of its first four postings, one byte each}, and
// after the list's entries (at byte 8 * n_buckets of its region) the in-bucket
// offset of every posting, one byte each, for buckets of more than four.  A
// probe reads one entry (a line covers 16 buckets: 4,096 docs at c = 8) and
// compares four bytes at once; a hit's posting index is rank + its position,
// and its tf comes from tf8 as for a bitmap.  A probe past the fourth posting
// of a larger bucket reads the next offset bytes (one 8-byte window: counts up
// to 9 cost no further wait); past the ninth it walks them.  A list whose
// postings crowd (more than 1/1024 of its buckets over kBucketWindow, as a
// topic-clustered term's do) keeps a bitmap: every wave would walk.
constexpr uint32_t kProbeShiftBit = 56;
constexpr uint64_t kProbeBaseMask = (1ull << kProbeShiftBit) - 1;
constexpr uint32_t kBucketDensity = 40;     // buckets below 2.5 % density, bitmaps above
constexpr uint32_t kBucketMinShift = 3, kBucketMaxShift = 8;
constexpr uint32_t kBucketInline = 4;       // offsets held in the entry
constexpr uint32_t kBucketWindow = 9;       // counts served without a walk
constexpr uint32_t kBucketCrowdedDiv = 1024;   // more crowded buckets than 1/this: a bitmap
inline uint32_t probe_shift(uint64_t bm) { return static_cast<uint32_t>(bm >> kProbeShiftBit); }
inline uint64_t bucket_count(uint32_t span, uint32_t c) { return (static_cast<uint64_t>(span) + (1u << c) - 1) >> c; }
// bucket shift for n postings over span docs (0: a bitmap): 1-2 postings per bucket
inline uint32_t bucket_shift(uint64_t n, uint32_t span) {
  // (ranks travel in 23 bits; a shard image's edge blocks add < 256 postings)
  if (!span || n * kBucketDensity >= span || n >= (1u << 23) - 1024) return 0;
  uint32_t c = kBucketMinShift;
  while (c < kBucketMaxShift && (n << (c + 1)) <= 2ull * span) ++c;   // doubled, the mean stays <= 2
  return c;
}
// words (u32) of a bucket list's region: entries, then one offset byte per posting
inline uint64_t bucket_words(uint64_t n, uint32_t span, uint32_t c) {
  return 2 * bucket_count(span, c) + (n + 7) / 8 * 2;
}

// Dense lists (df >= span / dense_div) also carry a rank bitmap of their doc
// ids over the image's doc range, so that a probe costs one load + a popcount
// instead of decoding the list's blocks.  The masks and the rank records are
// two arrays at the same index: DenseEnt = the 32-doc mask word (bit
// (d - doc_lo) % 32 of doc d), HostImage::dense_rank = per entry an 8-byte
// rank record {postings of the list (in the image's blocks) before the
// entry's first doc, the 1-byte tfs of the word's first four postings (255:
// more, or tf >= 255: read tf8)}; posting index = rank + popcount of the lower
// bits, block = index / 128.  The lean kernel's probe of the most selective
// other list reads the mask word alone (a 128-byte line covers 1,024 docs) and
// only a hit reads its rank record, whose tf bytes give the hit's tf in the
// same line.  At the en-Wikipedia shape a high-df driver's postings are ~180
// docs apart, so with the ranks beside the masks (8 bytes per 32 docs, 512
// docs per line) nearly every probe fetched a line of its own from HBM, and
// those line fetches bound the lean kernel (profiles/r03_probe_sweep.jsonl:
// ~12 CU-cycles per HBM line; r03_probe_forms.txt).  Other users (further
// lists, the general kernel) load both words at once: one probe = two
// independent loads.
constexpr uint32_t kDenseDocs = 32;   // doc ids per DenseEnt
struct DenseEnt {
  uint32_t w;        // bit (d - doc_lo) % 32 of doc d; its rank record: HostImage::dense_rank, same index
};
static_assert(sizeof(DenseEnt) == 4, "DenseEnt layout");
constexpr uint32_t kRankWords = 2;                          // u32 per rank record
constexpr uint64_t kDenseEntBytes = 4 + 4 * kRankWords;     // mask + rank record

// Host form of an entry's bit test and rank (the kernels have their own).
inline bool dense_ent_bit(const DenseEnt& e, uint32_t sh) { return (e.w >> sh) & 1u; }
inline uint32_t dense_ent_rank(const DenseEnt& e, uint32_t rank, uint32_t sh) {   // postings before bit sh
  return rank + static_cast<uint32_t>(__builtin_popcount(e.w & ((1u << sh) - 1u)));
}

// One 128-posting block (= one skip-list row, flash_containers.h:312-350).
struct BlockDev {
  uint32_t prev;      // previous_doc_id: delta seed, doc id of posting 128*i - 1
  uint32_t last;      // doc id of the block's last posting
  uint32_t doc_rel;   // docid blob offset relative to ListDev::base
  uint32_t tf_rel;    // tf blob offset relative to ListDev::base
};
static_assert(sizeof(BlockDev) == 16, "BlockDev layout");

struct QueryIn {
  int32_t n_terms;          // 0 => empty result
  int32_t k;                // n_results (0 => empty result)
  int32_t list[kMaxTerms];  // list ids in query order; -1 => term missing => empty
  int32_t flags;            // kQueryPhrase: SearchQuery::is_phrase (types.h:205-256)
  uint32_t ext;             // n_terms > kMaxTerms: all n_terms list ids are at
                            // reinterpret_cast<const int32_t*>(batch's QueryIn array) + ext
};
static_assert(sizeof(QueryIn) == 80, "QueryIn layout");
constexpr int32_t kQueryPhrase = 1;

// Planning constants of the device plan (plan_query_kernel) that the host's
// upload plan (batch_plan.cc) sizes the grids and workspaces by.
constexpr int kLeanWaves = 4;   // independent waves per lean_kernel workgroup
// Target block decodes per work item, for every class (lean, general,
// phrase); bounds seg_blocks (< 64).  Phrase items have been this long since
// round 3 (5 blocks before, while every conjunctive survivor ran the position
// check; now only the running top-k's candidates do, and longer items prune
// more: C5 leg 3.50 -> 4.95 M q/s at 63 blocks, 16: 4.27, 32: 4.56 M,
// profiles/r03_phrase_item_ab.txt).
constexpr int kSegCost = 63;
static_assert(kSegCost < 64, "a segment's driver directory is one entry per lane");
// A single-term item spans up to this many items' worth of blocks, which
// single_segment runs window by window: most of its blocks are skipped by
// their block bounds, so a short item would be mostly fixed cost.
constexpr int kSingleWindows = 8;

// The class rule, stated once for the device plan and the kernels
// (kernels.hip) and for the host's upload plan (batch_plan.cc); constexpr, so
// callable from device code.  A query's driver is its list of the fewest
// blocks here (the first of equals).
// Other list B is probed through its bitmap or buckets when it has them and is
// at least dense_ratio times as long as the driver (then a block decode per
// probe would mostly decode postings nobody asks for).  Image: what holds the
// engine's dense_ratio (the kernels' IndexArgs, the host plan's ImageView).
template <class Image>
constexpr bool probe_by_bitmap(const Image& ix, bool has_bm, uint32_t nblk_b, uint32_t nblk_driver) {
  return has_bm && static_cast<float>(nblk_b) >= ix.dense_ratio * static_cast<float>(nblk_driver);
}
// A one-term "phrase" is a plain term.
constexpr bool is_phrase_query(int32_t n_terms, int32_t flags) { return n_terms > 1 && (flags & kQueryPhrase); }
// Lean (lean_kernel; the rest: segment_kernel): every other list probed by
// bitmap, and not a phrase of more than two terms (the lean kernel checks
// positions of two-term phrases only, in registers).
constexpr bool is_lean_query(bool others_by_bitmap, int32_t n_terms, int32_t flags) {
  return others_by_bitmap && !(n_terms > 2 && (flags & kQueryPhrase));
}
// Tiny (tiny_kernel; the rule comes before the other two): a conjunctive
// query of two terms with k <= kMaxK whose lists are each, in this image, one
// VInts block, which the loader has decoded (ListDev::tail): two sorted arrays
// of at most 127 doc ids, met by one wave with no directory and no decode.
// Only plain runs have the class: in a shard step, and in a run that carries
// an owner replay, these queries stay with the other two classes.
constexpr bool is_tiny_list(uint32_t nblk, uint64_t tail) { return nblk == 1 && tail != kNoTail; }
constexpr bool is_tiny_query(int32_t n_terms, int32_t flags, int32_t k, bool tiny_list0, bool tiny_list1) {
  return n_terms == 2 && !(flags & kQueryPhrase) && k <= kMaxK && tiny_list0 && tiny_list1;
}

// Positions of one posting list in the image (phrase queries).  The list's
// position cozy box (flash_engine_dumper.h:78-104: full packs of 128 entries,
// then one VInts blob) is copied byte-identical to pos_blob at `base`; pack i
// starts at base + pos_pk[pk0 + i].x and has bit width pos_pk[pk0 + i].y; the
// VInts remainder is decoded at load (pos_tail[tail ..]).  Entry e of the box
// is in pack e / 128 when e < 128 * npk.  The bag of posting p (tf entries,
// delta coded from 0, flash_iterators.h:593-604) starts at entry
// pos_start[image slot of p] (slots as plen: 128 per image block).
struct PosDev {
  uint64_t base;
  uint64_t tail;
  uint32_t pk0;
  uint32_t npk;
};
static_assert(sizeof(PosDev) == 24, "PosDev layout");

// Written by the plan kernel for every query of a batch.
struct QueryPlan {
  uint32_t item_base;   // first work item of this query
  uint32_t n_items;     // segments (0 for empty queries)
  uint32_t seg_blocks;  // driver blocks per segment
  uint32_t driver;      // query slot of the shortest list (bits 0-7) | item cost bucket << 8
  uint64_t ev_base;     // first event slot (capacity = driver blocks * 128)
};
static_assert(sizeof(QueryPlan) == 24, "QueryPlan layout");

// Per-query work description of a lean query (every other list probed by
// bitmap, or a single term), written by the plan kernels so that a lean item's
// setup is one load of this record.
struct QueryDesc {
  uint64_t a_base;      // driver: blob base of its [docid | tf] span
  uint64_t a_tail;      //   decoded VInts last block (ListDev::tail)
  uint64_t o_bm;        // O1 (the other list with the fewest blocks): first bitmap entry
  uint64_t o_tf8;       //   offset of its 1-byte tfs
  uint64_t ev_base;     // = QueryPlan::ev_base
  uint32_t a_d16;       // driver: first block of its run in doc16 (kNoDoc16: decode its packs)
  uint32_t rsv0;
  uint64_t rsv1;
  double a_idf, o_idf;
  uint32_t a_blk0, a_nblk, a_tail_cnt;
  uint32_t min_last;    // smallest last doc id over the other lists
  uint32_t item_base, n_items, seg;
  uint32_t slots;       // driver slot | O1 slot << 16 (kNoSlot: single term)
  uint32_t o_list;      // O1's list id
  uint32_t k;           // n_results (> kMaxK: wide, every survivor is an event)
  // score bound of a driver posting before the other lists are probed (f32,
  // the lean kernel's pre-probe pruning): b_id * tf / (tf + norm) is its own
  // term (b_id = 2.2 * idf), b_iom / (b_m + norm) bounds all the other terms
  // (b_m = their largest tfmax, b_iom = sum of 2.2 * idf over them, times b_m)
  float b_id, b_iom, b_m;
  uint32_t nt;          // n_terms
};
static_assert(sizeof(QueryDesc) == 128, "QueryDesc layout");
constexpr uint32_t kNoSlot = 0xFFFFu;

// Disjunctive (OR) queries (wsr_query.flags & WSR_QUERY_OR) live in a table of
// their own: the QueryIn the conjunctive plan and kernels see shows them as
// empty queries.  The host resolves the terms (missing ones dropped), cuts the
// image's doc range into work items of about IndexArgs::seg_cap blocks over
// all of the query's lists, and sizes each item's event slot for its worst case.
constexpr int32_t kQueryOr = 2;
constexpr int kMaxOrTerms = 16;           // terms of an OR query (the ids held inline)
constexpr uint32_t kOrWindow = 2048;      // docs of or_kernel's accumulator window (a power of two)
struct OrQuery {
  int32_t q;            // the query's index in the batch (its hits row)
  int32_t k;            // n_results (> 0)
  int32_t nt;           // resolved terms (> 0)
  uint32_t item_base;   // first of its items in the OrItem table
  uint32_t n_items;
  uint32_t pad;
  int32_t list[kMaxOrTerms];    // list ids of the resolved terms, in query order
  double ubsum[kMaxOrTerms];    // MaxScore: the sum of the score bounds (2.2 * idf) of term t and
                                // of every term that sorts before it by (bound, slot)
};
static_assert(sizeof(OrQuery) == 216, "OrQuery layout");
struct OrItem {
  uint32_t oq;          // its query's entry in the OrQuery table
  uint32_t doc_lo, doc_hi;   // the item's docs: [doc_lo, doc_hi)
  uint32_t ev_cap;      // events its slot holds
  uint64_t ev_base;     // first event of its slot
};
static_assert(sizeof(OrItem) == 24, "OrItem layout");
// or_kernel's counters (wsr_or_stats), one u64 each
enum { kOrStatItems = 0, kOrStatWindows, kOrStatSkipped, kOrStatTouched, kOrStatEvents, kNumOrStats };

// Boolean queries (wsr_search_bool): the OR traversal plus, per doc, which
// term slots held it, and a predicate on that record.  A query's device record
// is an OrQuery (its resolved slots in query order, what or_replay_kernel
// reads, and the MaxScore sums over its MUST and SHOULD slots; a MUST_NOT
// slot's is 0.0) and, at the same place of a second table, its BoolRoles.
// Slots that can never hold a doc (a SHOULD or MUST_NOT term that is missing
// or has no block in the image) are dropped by the host, so the masks are over
// the resolved slots; need_should keeps counting the query's own slots.
struct BoolRoles {
  uint32_t must_mask, should_mask, not_mask;   // bit t: resolved slot t's role
  uint32_t need_should;   // SHOULD slots that must hold a doc: max(min_should, no MUST term ? 1 : 0)
  int32_t lead;           // the MUST slot with the fewest blocks in the image (-1: no MUST term)
};
static_assert(sizeof(BoolRoles) == 20, "BoolRoles layout");

// Scoring given (query, doc) pairs (wsr_score_docs): the host sorts each
// query's candidates by doc id and cuts them into items of at most
// kScoreLanes consecutive sorted candidates (score_plan.h); score_docs_kernel
// runs one wave per item, one candidate per lane.
constexpr uint32_t kScoreLanes = 64;
struct ScoreQuery {
  int32_t nt;                // terms of the query (its mask bits)
  int32_t list[kMaxTerms];   // list id per term, in query order; -1: no postings of it in this image
};
static_assert(sizeof(ScoreQuery) == 68, "ScoreQuery layout");
struct ScoreItem {
  uint32_t q;       // its query's entry in the ScoreQuery table
  uint32_t first;   // first of its candidates in the sorted doc and index arrays
  uint32_t n;       // candidates (1 .. kScoreLanes)
};
static_assert(sizeof(ScoreItem) == 12, "ScoreItem layout");
struct DocScore {   // = wsr_doc_score
  double score;
  uint32_t mask;
  int32_t pad;
};
static_assert(sizeof(DocScore) == 16, "DocScore layout");

// A heap-insertion event: a survivor that a top-k heap run from empty over its
// segment inserts (query_processing.h:595-602).
struct Event {
  double score;
  int32_t doc;
  int32_t pad;
};
static_assert(sizeof(Event) == 16, "Event layout");

struct HitDev {
  int32_t doc;
  int32_t pad;
  double score;
};
static_assert(sizeof(HitDev) == 16, "HitDev layout");

// The owner side of a doc-range shard exchange: this rank's nq queries of a
// batch, from q0, replayed over what every shard sent for them (built by
// owner_job_of, shard_layout.h; read by owner_replay_meta_kernel and, carried
// in FusedReplay, by a lean kernel's tail: kernels.h).
struct OwnerJob {
  const QueryIn* qs;      // the replayed batch's queries; owned ones from q0
  const int32_t* meta;    // {count, offset} of owned query i from shard g at meta + g * meta_stride + 2 * i
  const Event* recv;      // shard g's events at recv + g * stride + offset
  HitDev* hits;
  int32_t* n_hits;
  uint32_t* counters;     // the replayed batch's (error flags)
  uint64_t meta_stride, stride;
  int32_t q0, nq, n_shards, hit_stride;
};

}  // namespace wiser
