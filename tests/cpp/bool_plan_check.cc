// CPU check of the wsr_search_bool plan in wiser_amd/csrc/bool_plan.cc
// (tests/test_bool_plan.py): over a hand-made image directory, the slot masks,
// lead and need_should; the queries settled on the host have no entry and no
// item; the MaxScore sums leave MUST_NOT slots out; the items tile the doc
// range with event slots sized by the blocks that overlap them, capped by the
// lead list's with a MUST term; every error code with its message.
// One "ok <case>" line per case; exit status 0.
#include "../../wiser_amd/csrc/bool_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

using namespace wiser;

namespace {

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "bool_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

void ok(const char* name) { std::printf("ok %s\n", name); }

// The image, by the last doc of every block: big (8 blocks), mid (3), small
// (1), none (no block here: a shard that holds no posting of it), two (2).
enum { kBig = 0, kMid, kSmall, kNone, kTwo, kLists };
struct Image {
  std::vector<ListDev> lists;
  std::vector<BlockDev> blocks;
  void add(double idf, std::initializer_list<uint32_t> lasts) {
    ListDev L{};
    L.blk0 = static_cast<uint32_t>(blocks.size());
    L.nblk = static_cast<uint32_t>(lasts.size());
    L.idf = idf;
    uint32_t prev = 0;
    for (uint32_t last : lasts) {
      BlockDev b{};
      b.prev = prev;
      b.last = last;
      blocks.push_back(b);
      prev = L.last = last;
    }
    lists.push_back(L);
  }
  Image() {
    add(1.0, {999, 1999, 2999, 3999, 4999, 5999, 6999, 7999});
    add(2.0, {2499, 4999, 7499});
    add(3.0, {3100});
    add(4.0, {});
    add(2.5, {999, 6500});
  }
  ImageView view(uint32_t lo = 0, uint32_t hi = 0xFFFFFFFFu) const {
    ImageView v;
    v.lists = lists.data();
    v.n_lists = lists.size();
    v.blocks = blocks.data();
    v.n_blocks = blocks.size();
    v.doc_lo = lo;
    v.doc_hi = hi;
    return v;
  }
  // blocks of list id that can hold a doc of [lo, hi), one by one
  uint64_t overlap(int32_t id, uint32_t lo, uint32_t hi) const {
    const ListDev& L = lists[id];
    uint64_t n = 0;
    for (uint32_t j = 0; j < L.nblk; ++j) {
      const uint32_t start = j ? blocks[L.blk0 + j - 1].last + 1 : 0u;
      if (start < hi && blocks[L.blk0 + j].last >= lo) ++n;
    }
    return n;
  }
};
const Image g_img;

constexpr uint8_t M = WSR_ROLE_MUST, S = WSR_ROLE_SHOULD, N = WSR_ROLE_MUST_NOT;
wsr_bool_query Q(std::initializer_list<std::pair<int32_t, uint8_t>> terms, int32_t min_should = 0, int32_t k = 10) {
  wsr_bool_query q{};
  q.n_terms = static_cast<int32_t>(terms.size());
  q.k = k;
  q.min_should = min_should;
  int t = 0;
  for (const auto& p : terms) {
    q.list_ids[t] = p.first;
    q.role[t++] = p.second;
  }
  return q;
}

int plan(const ImageView& v, const std::vector<wsr_bool_query>& qs, BoolPlan* p, std::string* err,
         uint32_t target = 4, int32_t stride = 10) {
  return plan_bool(v, qs.data(), static_cast<int32_t>(qs.size()), stride, true, target, p, err);
}

// the properties of every planned query's items
void check_items(const ImageView& v, const BoolPlan& p) {
  CHECK(p.qs.size() == p.roles.size());
  uint64_t ev = 0;
  size_t at = 0;
  for (size_t i = 0; i < p.qs.size(); ++i) {
    const OrQuery& q = p.qs[i];
    const BoolRoles& r = p.roles[i];
    CHECK(q.item_base == at && q.n_items > 0);
    CHECK((r.must_mask | r.should_mask | r.not_mask) == (1u << q.nt) - 1u);
    CHECK(!(r.must_mask & r.should_mask) && !(r.must_mask & r.not_mask) && !(r.should_mask & r.not_mask));
    uint32_t top = 0;
    for (int t = 0; t < q.nt; ++t) top = std::max(top, g_img.lists[q.list[t]].last + 1);
    uint32_t pos = v.doc_lo;
    for (uint32_t j = 0; j < q.n_items; ++j, ++at) {
      const OrItem& it = p.items[at];
      CHECK(it.oq == i && it.doc_lo < it.doc_hi && it.doc_lo >= pos && it.doc_hi <= std::min(v.doc_hi, top));
      // (a gap before an item: docs that no block of the query's lists -- of its lead list -- can hold)
      uint64_t gap = 0, blocks = 0;
      for (int t = 0; t < q.nt; ++t) {
        if (it.doc_lo > pos && (r.lead < 0 || t == r.lead)) gap += g_img.overlap(q.list[t], pos, it.doc_lo);
        blocks += g_img.overlap(q.list[t], it.doc_lo, it.doc_hi);
      }
      CHECK(gap == 0);
      uint64_t cap = std::min<uint64_t>(it.doc_hi - it.doc_lo, 128 * blocks);
      if (r.lead >= 0) {
        const uint64_t lead = g_img.overlap(q.list[r.lead], it.doc_lo, it.doc_hi);
        CHECK(lead > 0);
        cap = std::min<uint64_t>(cap, 128 * lead);
      }
      CHECK(it.ev_cap == cap && it.ev_base == ev);
      ev += cap;
      pos = it.doc_hi;
    }
    const uint32_t end = std::min(v.doc_hi, top);
    for (int t = 0; t < q.nt; ++t)
      if (pos < end && (r.lead < 0 || t == r.lead)) CHECK(g_img.overlap(q.list[t], pos, end) == 0);
  }
  CHECK(at == p.items.size() && ev == p.ev_total);
}

void roles() {
  BoolPlan p;
  std::string err;
  // a missing SHOULD term and one without a block here are dropped; so is a missing MUST_NOT term
  CHECK(plan(g_img.view(), {Q({{kMid, M}, {kBig, S}, {-1, S}, {kSmall, N}, {kNone, S}, {kTwo, S}, {-1, N}}, 1),
                            Q({{kBig, M}, {kTwo, M}, {kMid, M}}, 0, 70), Q({{kSmall, S}, {kSmall, S}}, 2)},
             &p, &err, 4, 70) == WSR_OK);
  CHECK(p.qs.size() == 3 && p.nt_max == 4 && p.narrow && p.wide);
  const OrQuery& a = p.qs[0];
  CHECK(a.q == 0 && a.k == 10 && a.nt == 4);
  CHECK(a.list[0] == kMid && a.list[1] == kBig && a.list[2] == kSmall && a.list[3] == kTwo);
  CHECK(p.roles[0].must_mask == 1u && p.roles[0].should_mask == 10u && p.roles[0].not_mask == 4u);
  CHECK(p.roles[0].need_should == 1 && p.roles[0].lead == 0);
  // MaxScore sums in ascending (bound, slot) order over big, mid and two; nothing for the MUST_NOT slot
  const double b_big = 2.2 * 1.0, b_mid = 2.2 * 2.0, b_two = 2.2 * 2.5;
  CHECK(a.ubsum[1] == b_big && a.ubsum[0] == b_big + b_mid && a.ubsum[3] == b_big + b_mid + b_two);
  CHECK(a.ubsum[2] == 0.0);
  // the lead: the MUST slot with the fewest blocks; no SHOULD slot needed beside a MUST term
  CHECK(p.qs[1].q == 1 && p.qs[1].k == 70 && p.roles[1].must_mask == 7u && p.roles[1].should_mask == 0u);
  CHECK(p.roles[1].lead == 1 && p.roles[1].need_should == 0);
  // a term given twice is two slots
  CHECK(p.qs[2].nt == 2 && p.roles[2].should_mask == 3u && p.roles[2].need_should == 2 && p.roles[2].lead == -1);
  check_items(g_img.view(), p);
  ok("roles");
}

void settled() {
  BoolPlan p;
  std::string err;
  CHECK(plan(g_img.view(), {Q({{-1, M}, {kBig, S}}),              // a missing MUST term
                            Q({{kNone, M}, {kBig, S}}),           // a MUST list with no block in the image
                            Q({{kBig, S}, {kMid, S}, {-1, S}}, 3),   // min_should above the resolvable SHOULD slots
                            Q({{kBig, M}, {kNone, S}}, 1),        // ... beside a MUST term
                            Q({{kBig, N}, {kMid, N}}),            // MUST_NOT only
                            Q({{-1, S}, {kNone, S}}),             // no SHOULD slot left
                            Q({}), Q({{kBig, S}}, 0, 0), Q({{kBig, S}}, 0, -5)},
             &p, &err) == WSR_OK);
  CHECK(p.qs.empty() && p.roles.empty() && p.items.empty() && p.ev_total == 0 && !p.narrow && !p.wide);
  // a settled query between two live ones: the live ones keep their rows
  CHECK(plan(g_img.view(), {Q({{kBig, S}}), Q({{-1, M}}), Q({{kMid, M}})}, &p, &err) == WSR_OK);
  CHECK(p.qs.size() == 2 && p.qs[0].q == 0 && p.qs[1].q == 2);
  check_items(g_img.view(), p);
  CHECK(plan(g_img.view(), {}, &p, &err) == WSR_OK && p.qs.empty());
  CHECK(plan_bool(g_img.view(), nullptr, 0, 0, false, 4, &p, &err) == WSR_OK);
  ok("settled");
}

void items() {
  BoolPlan p;
  std::string err;
  // all SHOULD: or_plan's cut -- 11 blocks, the longest list has 8, 4 blocks per item: every 2nd block of big
  CHECK(plan(g_img.view(), {Q({{kBig, S}, {kMid, S}})}, &p, &err) == WSR_OK);
  CHECK(p.items.size() == 4);
  for (uint32_t j = 0; j < 4; ++j) CHECK(p.items[j].doc_lo == 2000 * j && p.items[j].doc_hi == 2000 * (j + 1));
  CHECK(p.items[0].ev_cap == 128 * 3 && p.items[1].ev_cap == 128 * 4);
  check_items(g_img.view(), p);
  // a MUST term: the items without a lead block go, the others are capped by the lead's blocks
  CHECK(plan(g_img.view(), {Q({{kSmall, M}, {kBig, S}}), Q({{kBig, N}, {kTwo, M}, {kMid, S}})}, &p, &err) == WSR_OK);
  CHECK(p.qs[0].n_items == 2 && p.items[0].doc_lo == 0 && p.items[0].doc_hi == 3000 && p.items[1].doc_hi == 6000);
  CHECK(p.items[0].ev_cap == 128 && p.items[1].ev_cap == 128 && p.items[1].ev_base == 128);
  CHECK(p.qs[1].item_base == 2 && p.ev_total > 256);
  check_items(g_img.view(), p);
  // one block per item, and a doc-range shard: the items stay inside the image's range
  for (uint32_t target : {1u, 63u}) {
    const ImageView v = g_img.view(2500, 5000);
    CHECK(plan(v, {Q({{kBig, S}, {kMid, S}, {kSmall, N}}), Q({{kMid, M}, {kBig, S}}), Q({{kTwo, M}, {kTwo, N}})},
               &p, &err, target) == WSR_OK);
    CHECK(p.qs.size() == 3 && p.items.front().doc_lo == 2500 && p.items[p.qs[0].n_items - 1].doc_hi == 5000);
    check_items(v, p);
  }
  ok("items");
}

void errors() {
  BoolPlan p;
  std::string err;
  const wsr_bool_query good = Q({{kBig, M}, {kMid, S}});
  auto refused = [&](wsr_bool_query bad, int code, const char* msg, int32_t stride = 10,
                     bool per_query = true) {
    err.clear();
    CHECK(plan(g_img.view(), {good, bad}, &p, &err, 4, stride) == code);
    CHECK(err == std::string("query 1: ") + msg);
    if (per_query) {   // (the per-query checks alone know nothing of a hit stride)
      std::string why;
      CHECK(check_bool_query(g_img.view(), bad, &why) == code && why == msg);
    }
  };
  wsr_bool_query b = good;
  b.n_terms = WSR_MAX_OR_TERMS + 1;
  refused(b, WSR_E_LIMIT, "a boolean query has at most WSR_MAX_OR_TERMS terms");
  b = good, b.k = WSR_MAX_K + 1;
  refused(b, WSR_E_LIMIT, "k over WSR_MAX_K", WSR_MAX_K + 1);
  b = good, b.k = 11;
  refused(b, WSR_E_LIMIT, "k over the call's hit stride", 10, false);
  b = good, b.role[1] = 3;
  refused(b, WSR_E_INVALID, "a term's role is none of WSR_ROLE_*");
  b = good, b.min_should = -1;
  refused(b, WSR_E_INVALID, "min_should is negative");
  b = good, b.n_terms = -1;
  refused(b, WSR_E_INVALID, "n_terms is negative");
  b = good, b.list_ids[0] = -2;
  refused(b, WSR_E_INVALID, "list id out of range");
  b = good, b.list_ids[1] = kLists;
  refused(b, WSR_E_INVALID, "list id out of range");
  // (what lies past n_terms is not read)
  b = good, b.role[2] = 9, b.list_ids[2] = 1 << 30;
  std::string why;
  CHECK(check_bool_query(g_img.view(), b, &why) == WSR_OK);
  // null arguments with nq > 0, a negative nq
  CHECK(plan_bool(g_img.view(), nullptr, 1, 10, true, 4, &p, &err) == WSR_E_INVALID && err == "bad arguments");
  CHECK(plan_bool(g_img.view(), &good, 1, 10, false, 4, &p, &err) == WSR_E_INVALID && err == "bad arguments");
  CHECK(plan_bool(g_img.view(), &good, -1, 10, true, 4, &p, &err) == WSR_E_INVALID && err == "bad arguments");
  // a refused plan holds nothing
  CHECK(p.qs.empty() && p.items.empty());
  ok("errors");
}

}  // namespace

int main() {
  roles();
  settled();
  items();
  errors();
  return 0;
}
