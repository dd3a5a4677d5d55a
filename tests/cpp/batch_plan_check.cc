// CPU check of the upload plan in wiser_amd/csrc/batch_plan.cc (tests/test_batch_plan.py):
// plan_upload, check_query and launches_of over a hand-made image directory,
// exact values for the instance flags, the class rule at its boundaries, the
// grids, the workspaces, long and disjunctive queries and the error returns.
// One "ok <case>" line per case; exit status 0.
#include "../../wiser_amd/csrc/batch_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

using namespace wiser;

namespace {

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      std::fprintf(stderr, "batch_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                     \
    }                                                                                   \
  } while (0)

void ok(const char* name) { std::printf("ok %s\n", name); }

// The image: list id -> blocks, probe structure, idf, last doc of block j.
//   0: no block here        1: 1 block, no bitmap (last 500)
//   2: 4 blocks, bitmap     (lasts 99, 199, 299, 399; idf 2)
//   3: 4 blocks, no bitmap  (lasts 149, 249, 349, 449; idf 1)
//   4: 5 blocks, bitmap     (lasts 49, 99, 149, 199, 249; idf 1)
//   5: 200 blocks, bitmap   (last of block j: 10 j + 9)
//   6: 600 blocks, bitmap   (last of block j: 5 j + 4)
//   7: 7 blocks, bitmap     8: 8 blocks, bitmap   (last of block j: 100 j + 99)
//   9: 600 blocks, no bitmap
// list_bytes[id] = 1000 + id, pos_bytes[id] = 10 + id.
enum { kEmpty = 0, kOne, kFourBm, kFour, kFive, k200, k600, kSeven, kEight, k600Plain, kLists };

struct Image {
  std::vector<ListDev> lists;
  std::vector<BlockDev> blocks;
  std::vector<uint64_t> list_bytes, pos_bytes;
  void add(uint32_t nblk, bool bm, double idf, uint32_t first_last, uint32_t step) {
    ListDev L{};
    L.blk0 = static_cast<uint32_t>(blocks.size());
    L.nblk = nblk;
    L.idf = idf;
    L.bm = bm ? 64 * lists.size() : kNoDense;
    for (uint32_t j = 0; j < nblk; ++j) {
      BlockDev b{};
      b.last = first_last + j * step;
      blocks.push_back(b);
      L.last = b.last;
    }
    list_bytes.push_back(1000 + lists.size());
    pos_bytes.push_back(10 + lists.size());
    lists.push_back(L);
  }
  Image() {
    add(0, true, 1.0, 0, 0);
    add(1, false, 3.0, 500, 0);
    add(4, true, 2.0, 99, 100);
    add(4, false, 1.0, 149, 100);
    add(5, true, 1.0, 49, 50);
    add(200, true, 0.5, 9, 10);
    add(600, true, 0.25, 4, 5);
    add(7, true, 1.0, 99, 100);
    add(8, true, 1.0, 99, 100);
    add(600, false, 0.25, 4, 5);
    CHECK(lists.size() == kLists);
  }
  ImageView view(float dense_ratio = 1.0f) const {
    ImageView v;
    v.lists = lists.data();
    v.n_lists = lists.size();
    v.blocks = blocks.data();
    v.n_blocks = blocks.size();
    v.list_bytes = list_bytes.data();
    v.pos_bytes = pos_bytes.data();
    v.dense_ratio = dense_ratio;
    v.doc_lo = 0;
    v.doc_hi = 3000;
    v.positions = true;
    v.lean_wgs = 100;
    v.lean_wgs_two = 110;
    v.lean_wgs_ph = 50;
    v.gen_cap = 40;
    return v;
  }
};
const Image g_img;
constexpr int32_t kStride = WSR_MAX_K;

wsr_query Q(std::initializer_list<int32_t> ids, int32_t k, int32_t flags = 0) {
  wsr_query q{};
  q.n_terms = static_cast<int32_t>(ids.size());
  q.k = k;
  q.flags = flags;
  int t = 0;
  for (int32_t id : ids) q.list_ids[t++] = id;
  return q;
}
constexpr int32_t PH = WSR_QUERY_PHRASE, OR = WSR_QUERY_OR;

UploadPlan plan(const ImageView& v, const std::vector<wsr_query>& qs, uint32_t seg_cap = kSegCost) {
  UploadPlan p;
  std::string err = "unset";
  const int rc = plan_upload(v, qs.data(), static_cast<int32_t>(qs.size()), kStride, seg_cap, &p, &err);
  if (rc != WSR_OK) std::fprintf(stderr, "batch_plan_check: plan_upload: %d %s\n", rc, err.c_str());
  CHECK(rc == WSR_OK && err == "unset");
  CHECK(p.in.size() == qs.size());
  return p;
}
BatchClass cls(const std::vector<wsr_query>& qs, float dense_ratio = 1.0f) {
  return plan(g_img.view(dense_ratio), qs).cls;
}

// the lean conjunctive / lean phrase / general driver blocks, read back from
// grids under caps that never bind (a grid of an empty class is 1, like one of need 1)
struct Needs {
  int lean, lean_ph, gen;
};
Needs needs(const std::vector<wsr_query>& qs, float dense_ratio = 1.0f) {
  ImageView v = g_img.view(dense_ratio);
  v.lean_wgs = v.lean_wgs_two = v.lean_wgs_ph = v.gen_cap = 1 << 30;
  const BatchClass c = plan(v, qs).cls;
  return Needs{c.has_conj_lean ? c.lean_wgs : 0, c.lean_wgs_ph, c.has_gen ? c.seg_grid : 0};
}

void instance_flags_case() {
  BatchClass c = cls({Q({kFourBm, kFive}, 10), Q({kFive, k200}, 64)});
  CHECK(c.two_conj && !c.one_conj && !c.has_wide && !c.has_phrase && c.two_ph);
  c = cls({Q({kFive}, 10), Q({k200}, 10)});
  CHECK(!c.two_conj && c.one_conj);
  // only empty / k <= 0 queries: the two-term instance
  c = cls({Q({}, 10), Q({kFive, kFourBm, k200}, 0), Q({kFive}, -1)});
  CHECK(c.two_conj && !c.one_conj);
  c = cls({});
  CHECK(c.two_conj && !c.one_conj && !c.has_conj_lean && !c.has_gen);
  // empty queries beside one-term / two-term ones leave the flag to those
  c = cls({Q({}, 10), Q({kFive}, 10)});
  CHECK(!c.two_conj && c.one_conj);
  c = cls({Q({kFive, k200, kFourBm}, 0), Q({kFive, k200}, 10)});
  CHECK(c.two_conj && !c.one_conj);
  // one three-term query clears both
  c = cls({Q({kFourBm, kFive}, 10), Q({kFourBm, kFive, k200}, 10)});
  CHECK(!c.two_conj && !c.one_conj);
  c = cls({Q({kFive}, 10), Q({kFourBm, kFive, k200}, 10)});
  CHECK(!c.two_conj && !c.one_conj);
  c = cls({Q({kFive}, 10), Q({kFourBm, kFive}, 10)});
  CHECK(!c.two_conj && !c.one_conj);
  // k at kMaxK
  c = cls({Q({kFourBm, kFive}, kMaxK)});
  CHECK(c.two_conj && !c.has_wide);
  c = cls({Q({kFourBm, kFive}, kMaxK + 1)});
  CHECK(!c.two_conj && !c.one_conj && c.has_wide);
  c = cls({Q({kFive}, kMaxK + 1)});   // (one_conj does not look at k)
  CHECK(!c.two_conj && c.one_conj && c.has_wide);
  // ... for two_ph on a phrase (neutral to the conjunctive flags)
  c = cls({Q({kFourBm, kFive}, kMaxK, PH)});
  CHECK(c.has_phrase && c.two_ph && !c.has_wide && c.two_conj && !c.one_conj);
  c = cls({Q({kFourBm, kFive}, kMaxK + 1, PH)});
  CHECK(c.has_phrase && !c.two_ph && c.has_wide && c.two_conj);
  c = cls({Q({kFourBm, kFive}, kMaxK + 1), Q({kFourBm, kFive}, kMaxK, PH)});   // a wide conjunctive query: two_ph stays
  CHECK(c.two_ph && !c.two_conj && c.has_wide);
  ok("instance_flags");
}

void class_rule_case() {
  // dense_ratio 1.0: an other list of exactly the driver's blocks is lean when it has a bitmap
  // (one block fewer and it is the driver itself: at 1.0 the rule is "has a bitmap")
  Needs n = needs({Q({kFour, kFourBm}, 10)});   // driver: the first of equals, kFour
  CHECK(n.lean == 1 && n.gen == 0);
  BatchClass c = cls({Q({kFour, kFourBm}, 10)});
  CHECK(c.has_conj_lean && !c.has_gen);
  n = needs({Q({kFourBm, kFour}, 10)});         // the other list has no bitmap
  CHECK(n.lean == 0 && n.gen == 4);
  c = cls({Q({kFourBm, kFour}, 10)});
  CHECK(!c.has_conj_lean && c.has_gen);
  // no bitmap: general whatever its length
  n = needs({Q({kFive, k600Plain}, 10)});
  CHECK(n.lean == 0 && n.gen == 5);
  n = needs({Q({kFive, k600}, 10)});
  CHECK(n.lean == 2 && n.gen == 0);   // (5 blocks: two workgroups of kLeanWaves)
  // every other list must pass
  n = needs({Q({kFive, k600, k600Plain}, 10)});
  CHECK(n.lean == 0 && n.gen == 5);
  n = needs({Q({kFive, k600, k200}, 10)});
  CHECK(n.lean == 2 && n.gen == 0);
  // dense_ratio 2.0, driver of 4 blocks: 8 blocks lean, 7 general
  n = needs({Q({kFour, kEight}, 10)}, 2.0f);
  CHECK(n.lean == 1 && n.gen == 0);
  n = needs({Q({kFour, kSeven}, 10)}, 2.0f);
  CHECK(n.lean == 0 && n.gen == 4);
  n = needs({Q({kFour, kFourBm}, 10)}, 2.0f);
  CHECK(n.lean == 0 && n.gen == 4);
  // dense_ratio 1.5, driver of 5 blocks (7.5): 8 lean, 7 general
  n = needs({Q({kFive, kEight}, 10)}, 1.5f);
  CHECK(n.lean == 2 && n.gen == 0);
  n = needs({Q({kFive, kSeven}, 10)}, 1.5f);
  CHECK(n.lean == 0 && n.gen == 5);
  // phrases: two terms in the phrase lean need, three in the general one
  n = needs({Q({kFive, k200}, 10, PH)});
  CHECK(n.lean == 0 && n.lean_ph == 2 && n.gen == 0);
  c = cls({Q({kFive, k200}, 10, PH)});
  CHECK(c.has_phrase && !c.gen_phrase && !c.has_conj_lean && !c.has_gen);
  n = needs({Q({kFive, k200, k600}, 10, PH)});
  CHECK(n.lean == 0 && n.lean_ph == 1 && n.gen == 5);
  c = cls({Q({kFive, k200, k600}, 10, PH)});
  CHECK(c.has_phrase && c.gen_phrase && !c.has_conj_lean && c.has_gen);
  n = needs({Q({kFive, k600Plain}, 10, PH)});   // a two-term phrase over a list without bitmap
  CHECK(n.lean_ph == 1 && n.gen == 5);
  CHECK(cls({Q({kFive, k600Plain}, 10, PH)}).gen_phrase);
  // a one-term "phrase" is conjunctive
  c = cls({Q({kFive}, 10, PH)});
  CHECK(!c.has_phrase && !c.gen_phrase && c.one_conj && c.has_conj_lean && !c.has_gen);
  UploadPlan p = plan(g_img.view(), {Q({kFive}, 10, PH), Q({kFive, k200}, 10, PH)});
  CHECK(p.in[0].flags == 0 && p.in[1].flags == kQueryPhrase);
  // algo_static: spans + 12 k; a phrase adds its position boxes (when the image has them)
  CHECK(cls({Q({kFive, k200}, 10)}).algo_static == 1004 + 1005 + 120);
  CHECK(cls({Q({kFive, k200}, 10, PH)}).algo_static == 1004 + 1005 + 14 + 15 + 120);
  ImageView v = g_img.view();
  v.pos_bytes = nullptr;
  CHECK(plan(v, {Q({kFive, k200}, 10, PH)}).cls.algo_static == 1004 + 1005 + 120);
  ok("class_rule");
}

void grids_case() {
  // max(1, min(cap, need)); the lean need in workgroups of kLeanWaves, rounded up
  BatchClass c = cls({});
  CHECK(c.seg_grid == 1 && c.lean_wgs == 1 && c.lean_wgs_ph == 1);
  c = cls({Q({kFive}, 10)});   // 5 blocks
  CHECK(c.lean_wgs == 2 && c.seg_grid == 1 && c.lean_wgs_ph == 1);
  c = cls({Q({kFourBm}, 10)});   // 4 blocks
  CHECK(c.lean_wgs == 1);
  c = cls({Q({k200}, 10), Q({k200}, 10)});   // 400 blocks: the cap of the one-term batch
  CHECK(c.one_conj && c.lean_wgs == 100);
  c = cls({Q({k200}, 10), Q({k200}, 10), Q({kFourBm, kFive, k600}, 10)});   // ... of a mixed batch
  CHECK(!c.one_conj && !c.two_conj && c.lean_wgs == 100);
  c = cls({Q({k200, k600}, 10), Q({k200, k600}, 10), Q({k200, k600}, 10)});   // two_conj: lean_wgs_two
  CHECK(c.two_conj && c.lean_wgs == 110);
  c = cls({Q({k200, k600}, 10), Q({k200, k600}, 10), Q({kFive, k600}, 10)});   // 405 blocks: 102 workgroups
  CHECK(c.two_conj && c.lean_wgs == 102);
  c = cls({Q({k200, k600Plain}, 10)});   // general: 200 blocks over the cap of 40
  CHECK(c.seg_grid == 40 && c.lean_wgs == 1);
  c = cls({Q({kFive, k600Plain}, 10), Q({kFour, k600Plain}, 10)});
  CHECK(c.seg_grid == 9);
  c = cls({Q({k200, k600}, 10, PH), Q({k200, k600}, 10, PH)});   // 400 blocks: the phrase cap
  CHECK(c.lean_wgs_ph == 50 && c.lean_wgs == 1 && c.seg_grid == 1);
  c = cls({Q({kFive, k600}, 10, PH), Q({kFour, k200}, 10, PH)});   // 9 blocks
  CHECK(c.lean_wgs_ph == 3);
  ok("grids");
}

void invalid_queries_case() {
  const int32_t out_of_range = kLists;
  for (int32_t bad : {-1, out_of_range, static_cast<int32_t>(kEmpty)}) {
    UploadPlan p = plan(g_img.view(), {Q({bad, k200}, 10), Q({k200, bad}, 10), Q({kFive, bad, k200}, 10, PH)});
    const BatchClass& c = p.cls;
    CHECK(p.ev_need == 0 && p.items_need == 0 && c.algo_static == 0);
    CHECK(!c.has_conj_lean && !c.has_gen && !c.gen_phrase);
    CHECK(c.seg_grid == 1 && c.lean_wgs == 1 && c.lean_wgs_ph == 1);
    CHECK(c.two_conj && !c.one_conj && c.has_phrase);   // by their term counts
    CHECK(p.in[0].n_terms == 2 && p.in[0].list[0] == bad && p.in[0].list[1] == k200 && p.in[0].list[2] == -1);
    p = plan(g_img.view(), {Q({bad}, 10), Q({kFive}, 10)});
    CHECK(p.cls.one_conj && !p.cls.two_conj && p.items_need == 5 && p.cls.algo_static == 1004 + 120);
    p = plan(g_img.view(), {Q({bad, kFive, k200}, 10), Q({kFive, k200}, 10)});
    CHECK(!p.cls.one_conj && !p.cls.two_conj && p.items_need == 5);
  }
  // k <= 0 and no terms: nothing either
  UploadPlan p = plan(g_img.view(), {Q({kFive, k200}, 0), Q({kFive}, -3), Q({}, 10)});
  CHECK(p.ev_need == 0 && p.items_need == 0 && p.cls.algo_static == 0 && !p.cls.has_conj_lean && !p.cls.has_gen);
  CHECK(p.in[0].k == 0 && p.in[1].k == 0 && p.in[1].n_terms == 1 && p.in[2].n_terms == 0 && p.in[2].k == 10);
  wsr_query neg = Q({}, 10);
  neg.n_terms = -2;
  p = plan(g_img.view(), {neg});
  CHECK(p.in[0].n_terms == 0 && p.cls.two_conj && p.items_need == 0);
  ok("invalid_queries");
}

void workspace_case() {
  // ev_need = (nbmin + seg_max) * 128; one term: seg_max = min(nbmin, kSegCost * kSingleWindows)
  UploadPlan p = plan(g_img.view(), {Q({kFive}, 10)});
  CHECK(p.ev_need == (5 + 5) * 128 && p.items_need == 5);
  p = plan(g_img.view(), {Q({k600}, 10)});
  CHECK(kSegCost * kSingleWindows == 504);
  CHECK(p.ev_need == (600 + 504) * 128 && p.items_need == 600);
  p = plan(g_img.view(), {Q({kFive, k600}, 10)});
  CHECK(p.ev_need == (5 + 63) * 128 && p.items_need == 5);
  p = plan(g_img.view(), {Q({k600, k600Plain}, 10)});
  CHECK(p.ev_need == (600 + 63) * 128 && p.items_need == 600);
  // seg_cap (the batch's item length) does not enter the conjunctive workspace
  p = plan(g_img.view(), {Q({k600}, 10)}, 8);
  CHECK(p.ev_need == (600 + 504) * 128);
  // sums over the batch
  p = plan(g_img.view(), {Q({kFive}, 10), Q({k600}, 10), Q({kFive, k600}, 10, PH), Q({kEmpty, k600}, 10)});
  CHECK(p.ev_need == (10 + 1104 + 68) * 128 && p.items_need == 5 + 600 + 5);
  CHECK(p.q_bytes == 4 * sizeof(QueryIn));
  ok("workspace");
}

void long_queries_case() {
  // 17 terms: list_ids hold 16, more_ids the rest; ext = the QueryIn array's words + terms before
  std::vector<int32_t> more_a = {kFive}, more_b = {k200, kEight, kSeven};
  wsr_query a = Q({k600, k600, k600, k600, k600, k600, k600, k600, k600, k600, k600, k600, k600, k600, k600, k200}, 10);
  a.n_terms = 17;
  a.more_ids = more_a.data();
  wsr_query b = a;
  b.n_terms = 19;
  b.list_ids[0] = k600Plain;
  b.more_ids = more_b.data();
  UploadPlan p = plan(g_img.view(), {Q({kFive}, 10), a, Q({kFive, k200}, 10), b});
  const uint32_t words = sizeof(QueryIn) * 4 / 4;
  CHECK(words == 80);
  CHECK(p.in[0].ext == 0 && p.in[2].ext == 0);
  CHECK(p.in[1].n_terms == 17 && p.in[1].ext == words);
  CHECK(p.in[3].n_terms == 19 && p.in[3].ext == words + 17);
  CHECK(p.ext.size() == 17 + 19 && p.q_bytes == 4 * sizeof(QueryIn) + 4 * 36);
  for (int t = 0; t < 16; ++t) {
    CHECK(p.in[1].list[t] == a.list_ids[t] && p.ext[t] == a.list_ids[t]);
    CHECK(p.in[3].list[t] == b.list_ids[t] && p.ext[17 + t] == b.list_ids[t]);
  }
  CHECK(p.ext[16] == kFive && p.ext[17 + 16] == k200 && p.ext[17 + 17] == kEight && p.ext[17 + 18] == kSeven);
  // the class rule reads every term: a's driver is its 17th (5 blocks, every other list a bitmap),
  // b's is the 7-block list and its first term has no bitmap
  CHECK(p.items_need == 5 + 5 + 5 + 7);
  CHECK(!p.cls.two_conj && !p.cls.one_conj && p.cls.has_conj_lean && p.cls.has_gen && p.cls.seg_grid == 7);
  CHECK(p.cls.lean_wgs == 4);   // 15 blocks
  CHECK(p.cls.algo_static == (1004 + 120) + (15 * 1006 + 1005 + 1004 + 120) + (1004 + 1005 + 120) +
                                 (1009 + 14 * 1006 + 1005 + 1005 + 1008 + 1007 + 120));
  // 16 terms stay inline
  a.n_terms = 16;
  p = plan(g_img.view(), {a});
  CHECK(p.ext.empty() && p.in[0].ext == 0 && p.in[0].list[15] == k200 && p.items_need == 200);
  ok("long_queries");
}

// the items of entry e of the table tile [lo, hi) in order
void check_tiles(const UploadPlan& p, size_t e, uint32_t lo, uint32_t hi) {
  const OrQuery& oq = p.orq[e];
  CHECK(oq.n_items > 0 && oq.item_base + oq.n_items <= p.or_items.size());
  for (uint32_t r = 0; r < oq.n_items; ++r) {
    const OrItem& it = p.or_items[oq.item_base + r];
    CHECK(it.oq == e && it.doc_lo < it.doc_hi);
    CHECK(it.doc_lo == (r ? p.or_items[oq.item_base + r - 1].doc_hi : lo));
  }
  CHECK(p.or_items[oq.item_base + oq.n_items - 1].doc_hi == hi);
}

void or_queries_case() {
  // neutral to every conjunctive flag, an empty QueryIn row; a wide one is not has_wide
  UploadPlan p = plan(g_img.view(), {Q({kFourBm, kFive}, 10), Q({kFourBm, kFour}, 100, OR)}, 4);
  CHECK(p.cls.two_conj && !p.cls.one_conj && !p.cls.has_wide && !p.cls.has_phrase && p.cls.two_ph);
  CHECK(p.cls.has_or && p.cls.or_wide && !p.cls.or_narrow && p.cls.n_or == 1);
  CHECK(p.cls.has_conj_lean && !p.cls.has_gen && p.items_need == 4 && p.ev_need == (4 + 63) * 128);
  CHECK(p.in[1].n_terms == 0 && p.in[1].k == 100 && p.in[1].flags == 0 && p.in[1].ext == 0);
  for (int t = 0; t < kMaxTerms; ++t) CHECK(p.in[1].list[t] == -1);
  p = plan(g_img.view(), {Q({kFive}, 10), Q({kFourBm, kFour, kFive}, 10, OR)});
  CHECK(p.cls.one_conj && !p.cls.two_conj && p.cls.or_narrow && !p.cls.or_wide);

  // A: lists 2 and 3 (a missing and a blockless term dropped), items of about 4 blocks;
  // B: list 4 alone, wide; C and D: nothing resolved / k 0 -- absent
  p = plan(g_img.view(), {Q({kFourBm, -1, kEmpty, kFour}, 10, OR), Q({kFive}, 100, OR), Q({-1, kEmpty}, 10, OR),
                          Q({kFourBm}, 0, OR), Q({}, 10, OR)},
           4);
  const BatchClass& c = p.cls;
  CHECK(c.has_or && c.n_or == 2 && p.orq.size() == 2 && c.or_items == 4 && p.or_items.size() == 4);
  CHECK(c.or_narrow && c.or_wide && c.or_nt_max == 2);
  CHECK(c.two_conj && !c.one_conj && !c.has_conj_lean && !c.has_gen && p.items_need == 0 && p.ev_need == 0);
  CHECK(c.algo_static == (1002 + 1003 + 120) + (1004 + 1200));
  const OrQuery& A = p.orq[0];
  CHECK(A.q == 0 && A.k == 10 && A.nt == 2 && A.list[0] == kFourBm && A.list[1] == kFour);
  CHECK(A.item_base == 0 && A.n_items == 2);
  // ubsum: ascending (bound, slot): slot 1 (idf 1), then slot 0 (idf 2)
  double s = 0.0;
  s += 2.2 * 1.0;
  CHECK(A.ubsum[1] == s);
  s += 2.2 * 2.0;
  CHECK(A.ubsum[0] == s);
  // step = 4 * 4 / 8 = 2 blocks of list 2: [0, 200) and [200, 450); 450 = one past the lists' last doc
  const OrItem* it = p.or_items.data();
  CHECK(it[0].oq == 0 && it[0].doc_lo == 0 && it[0].doc_hi == 200 && it[0].ev_cap == 200 && it[0].ev_base == 0);
  CHECK(it[1].oq == 0 && it[1].doc_lo == 200 && it[1].doc_hi == 450 && it[1].ev_cap == 250 && it[1].ev_base == 200);
  const OrQuery& B = p.orq[1];
  CHECK(B.q == 1 && B.k == 100 && B.nt == 1 && B.list[0] == kFive && B.item_base == 2 && B.n_items == 2);
  CHECK(B.ubsum[0] == 2.2 * 1.0);
  // step 4: [0, 200) over 4 blocks, [200, 250) over one: ev_base goes on across queries
  CHECK(it[2].oq == 1 && it[2].doc_lo == 0 && it[2].doc_hi == 200 && it[2].ev_cap == 200 && it[2].ev_base == 450);
  CHECK(it[3].oq == 1 && it[3].doc_lo == 200 && it[3].doc_hi == 250 && it[3].ev_cap == 50 && it[3].ev_base == 650);
  CHECK(p.or_ev == 700);
  check_tiles(p, 0, 0, 450);
  check_tiles(p, 1, 0, 250);

  // ev_cap = 128 * blocks where that is the smaller: 1 block over 500 docs
  p = plan(g_img.view(), {Q({kOne}, 10, OR)});
  CHECK(p.or_items.size() == 1 && p.or_items[0].doc_lo == 0 && p.or_items[0].doc_hi == 501);
  CHECK(p.or_items[0].ev_cap == 128 && p.or_ev == 128);

  // an image of docs [120, 420): the items are clipped to it
  ImageView v = g_img.view();
  v.doc_lo = 120;
  v.doc_hi = 420;
  p = plan(v, {Q({kFourBm, kFour}, 10, OR)}, 4);
  it = p.or_items.data();
  CHECK(p.or_items.size() == 2);
  CHECK(it[0].doc_lo == 120 && it[0].doc_hi == 200 && it[0].ev_cap == 80 && it[0].ev_base == 0);
  CHECK(it[1].doc_lo == 200 && it[1].doc_hi == 420 && it[1].ev_cap == 220 && it[1].ev_base == 80);
  check_tiles(p, 0, 120, 420);

  // ties of the bound keep slot order: lists 2 (idf 2), 3 and 4 (idf 1): slots 1, 2, 0
  p = plan(g_img.view(), {Q({kFourBm, kFour, kFive}, 10, OR)});
  CHECK(p.cls.or_nt_max == 3);
  s = 2.2 * 1.0;
  CHECK(p.orq[0].ubsum[1] == s);
  s += 2.2 * 1.0;
  CHECK(p.orq[0].ubsum[2] == s);
  s += 2.2 * 2.0;
  CHECK(p.orq[0].ubsum[0] == s);
  check_tiles(p, 0, 0, 450);

  // long lists at the default item length: tiles, slots back to back
  p = plan(g_img.view(), {Q({k200, k600, kSeven}, 10, OR), Q({k600, k600Plain}, 65, OR)});
  check_tiles(p, 0, 0, 3000);
  check_tiles(p, 1, 0, 3000);
  CHECK(p.orq[0].n_items > 1 && p.orq[1].item_base == p.orq[0].n_items);
  uint64_t ev = 0;
  for (const OrItem& i : p.or_items) {
    CHECK(i.ev_base == ev && i.ev_cap > 0 && i.ev_cap <= i.doc_hi - i.doc_lo);
    ev += i.ev_cap;
  }
  CHECK(ev == p.or_ev && p.cls.or_items == p.or_items.size());
  ok("or_queries");
}

void expect_error(const ImageView& v, const std::vector<wsr_query>& qs, int32_t stride, int code, const char* msg) {
  UploadPlan p;
  std::string err;
  const int rc = plan_upload(v, qs.data(), static_cast<int32_t>(qs.size()), stride, kSegCost, &p, &err);
  if (rc != code || err != msg) std::fprintf(stderr, "batch_plan_check: got %d \"%s\"\n", rc, err.c_str());
  CHECK(rc == code && err == msg);
}

void errors_case() {
  const ImageView v = g_img.view();
  const wsr_query good = Q({kFive}, 10);
  expect_error(v, {good, Q({kFive}, 11)}, 10, WSR_E_LIMIT, "query 1: k over the batch's hit stride");
  expect_error(v, {Q({kFive, k200}, 10, OR | PH)}, kStride, WSR_E_INVALID,
               "query 0: a query is a phrase or a disjunction, not both");
  wsr_query q = Q({kFive}, 10, OR);
  q.n_terms = WSR_MAX_OR_TERMS + 1;
  std::vector<int32_t> more(WSR_MAX_QUERY_TERMS, kFive);
  q.more_ids = more.data();
  expect_error(v, {good, good, q}, kStride, WSR_E_LIMIT,
               "query 2: a disjunctive query has at most WSR_MAX_OR_TERMS terms");
  q = Q({kFive}, 10);
  q.n_terms = WSR_MAX_TERMS + 1;
  expect_error(v, {q}, kStride, WSR_E_INVALID, "query 0: a query of more than WSR_MAX_TERMS terms needs more_ids");
  ImageView nopos = v;
  nopos.positions = false;
  nopos.pos_bytes = nullptr;
  expect_error(nopos, {good, Q({kFive, k200}, 10, PH)}, kStride, WSR_E_INVALID,
               "query 1: phrase query on an engine opened without positions");
  CHECK(plan(nopos, {Q({kFive}, 10, PH)}).cls.one_conj);   // (a one-term "phrase" needs none)
  // the rest of wsr_check_query's rule
  q = Q({kFive}, 10);
  q.n_terms = WSR_MAX_QUERY_TERMS + 1;
  q.more_ids = more.data();
  expect_error(v, {q}, kStride, WSR_E_LIMIT, "query 0: n_terms or k over the limit");
  expect_error(v, {Q({kFive}, 10, 4)}, kStride, WSR_E_INVALID, "query 0: unknown flags");
  q = Q({kFive}, 10, PH);
  q.n_terms = WSR_MAX_PHRASE_TERMS + 1;
  expect_error(v, {q}, kStride, WSR_E_LIMIT, "query 0: a phrase query has at most WSR_MAX_PHRASE_TERMS terms");
  // a disjunctive query's ids: -1 is a missing term, every other id outside the lists an error
  expect_error(v, {Q({kFive, kLists}, 10, OR)}, kStride, WSR_E_INVALID, "query 0: list id out of range");
  expect_error(v, {good, Q({-2}, 0, OR)}, kStride, WSR_E_INVALID, "query 1: list id out of range");
  // check_query alone: no prefix
  std::string err;
  CHECK(check_query(v, Q({kFive, k200}, 10, OR | PH), &err) == WSR_E_INVALID);
  CHECK(err == "a query is a phrase or a disjunction, not both");
  CHECK(check_query(v, Q({kFive}, WSR_MAX_K + 1), &err) == WSR_E_LIMIT && err == "n_terms or k over the limit");
  err = "unset";
  CHECK(check_query(v, Q({kFive, -1}, WSR_MAX_K, PH), &err) == WSR_OK && err == "unset");
  ok("errors");
}

void launches_case() {
  for (int m = 0; m < 32; ++m) {
    BatchClass c;
    c.has_phrase = m & 1;
    c.has_conj_lean = m & 2;
    c.has_gen = m & 4;
    const bool step = m & 8, carried = m & 16;
    const Launches l = launches_of(c, step, carried);
    // without a phrase query, in a shard step: everything; else what the class rule found,
    // and the conjunctive launch also for a carried owner replay
    const bool all = step || !c.has_phrase;
    CHECK(l.conj == (all || carried || c.has_conj_lean));
    CHECK(l.gen == (all || c.has_gen));
  }
  BatchClass c;   // a few rows spelled out
  c.has_phrase = true;
  c.has_conj_lean = c.has_gen = false;
  CHECK(!launches_of(c, false, false).conj && !launches_of(c, false, false).gen);
  CHECK(launches_of(c, false, true).conj && !launches_of(c, false, true).gen);
  CHECK(launches_of(c, true, false).conj && launches_of(c, true, false).gen);
  c.has_gen = true;
  CHECK(!launches_of(c, false, false).conj && launches_of(c, false, false).gen);
  c.has_phrase = false;
  c.has_gen = false;
  CHECK(launches_of(c, false, false).conj && launches_of(c, false, false).gen);
  const BatchClass fresh;   // a batch before its first upload launches everything
  CHECK(launches_of(fresh, false, false).conj && launches_of(fresh, false, false).gen);
  CHECK(Launches().conj && Launches().gen);
  ok("launches_of");
}

void reuse_case() {
  // a plan object planned into twice holds the second plan only
  UploadPlan p;
  std::string err;
  const std::vector<wsr_query> a = {Q({kFourBm, kFour}, 100, OR), Q({kFive, k600Plain}, 100, PH)};
  const std::vector<wsr_query> b = {Q({kFive}, 10)};
  CHECK(plan_upload(g_img.view(), a.data(), 2, kStride, kSegCost, &p, &err) == WSR_OK);
  CHECK(p.cls.has_or && p.cls.has_phrase && p.cls.gen_phrase && p.cls.has_wide && !p.or_items.empty());
  CHECK(plan_upload(g_img.view(), b.data(), 1, kStride, kSegCost, &p, &err) == WSR_OK);
  const UploadPlan f = plan(g_img.view(), b);
  CHECK(p.in.size() == 1 && p.ext.empty() && p.orq.empty() && p.or_items.empty() && p.or_ev == 0);
  CHECK(p.ev_need == f.ev_need && p.items_need == f.items_need && p.q_bytes == f.q_bytes);
  CHECK(!p.cls.has_or && !p.cls.has_phrase && !p.cls.gen_phrase && !p.cls.has_wide && p.cls.one_conj);
  CHECK(p.cls.n_or == 0 && p.cls.or_items == 0 && p.cls.or_nt_max == 0 && p.cls.algo_static == f.cls.algo_static);
  ok("reuse");
}

}  // namespace

int main() {
  instance_flags_case();
  class_rule_case();
  grids_case();
  invalid_queries_case();
  workspace_case();
  long_queries_case();
  or_queries_case();
  errors_case();
  launches_case();
  reuse_case();
  return 0;
}
