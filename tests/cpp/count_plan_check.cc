// CPU check of the wsr_count_bool plan, plan_count in
// wiser_amd/csrc/bool_plan.cc (tests/test_count_plan.py): over a hand-made
// image directory, k is ignored (any k plans the same, none is refused or
// settled); the queries settled on the host; the items are plan_bool's for the
// same query, without event slots; every error code with its message.
// One "ok <case>" line per case; exit status 0.
#include "../../wiser_amd/csrc/bool_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

using namespace wiser;

namespace {

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      std::fprintf(stderr, "count_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                     \
    }                                                                                   \
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

int count_plan(const ImageView& v, const std::vector<wsr_bool_query>& qs, BoolPlan* p, std::string* err,
               uint32_t target = 4) {
  return plan_count(v, qs.data(), static_cast<int32_t>(qs.size()), true, target, p, err);
}

// the live queries of the cases below: every role, a dropped slot, a lead that loses items
std::vector<wsr_bool_query> live(int32_t k) {
  return {Q({{kBig, S}, {kMid, S}}, 0, k),
          Q({{kMid, M}, {kBig, S}, {-1, S}, {kSmall, N}, {kNone, S}, {kTwo, S}, {-1, N}}, 1, k),
          Q({{kSmall, M}, {kBig, S}}, 0, k),
          Q({{kBig, N}, {kTwo, M}, {kMid, S}}, 0, k),
          Q({{kSmall, S}, {kSmall, S}}, 2, k)};
}

bool same_tables(const BoolPlan& a, const BoolPlan& b, bool with_k) {
  if (a.qs.size() != b.qs.size() || a.items.size() != b.items.size() || a.nt_max != b.nt_max) return false;
  for (size_t i = 0; i < a.qs.size(); ++i) {
    const OrQuery &x = a.qs[i], &y = b.qs[i];
    const BoolRoles &r = a.roles[i], &s = b.roles[i];
    if (x.q != y.q || x.nt != y.nt || x.item_base != y.item_base || x.n_items != y.n_items) return false;
    if (with_k && x.k != y.k) return false;
    for (int t = 0; t < x.nt; ++t)
      if (x.list[t] != y.list[t]) return false;
    if (r.must_mask != s.must_mask || r.should_mask != s.should_mask || r.not_mask != s.not_mask ||
        r.need_should != s.need_should || r.lead != s.lead)
      return false;
  }
  for (size_t j = 0; j < a.items.size(); ++j)
    if (a.items[j].oq != b.items[j].oq || a.items[j].doc_lo != b.items[j].doc_lo ||
        a.items[j].doc_hi != b.items[j].doc_hi)
      return false;
  return true;
}

void k_ignored() {
  BoolPlan ref, p;
  std::string err;
  CHECK(count_plan(g_img.view(), live(10), &ref, &err) == WSR_OK);
  CHECK(ref.qs.size() == 5 && !ref.items.empty());
  // zero, negative, above WSR_MAX_K: neither refused nor settled, and the same plan
  for (int32_t k : {0, -5, 1, WSR_MAX_K, WSR_MAX_K + 1, 5000, 0x7FFFFFFF}) {
    CHECK(count_plan(g_img.view(), live(k), &p, &err) == WSR_OK);
    CHECK(same_tables(ref, p, true));
    for (const OrQuery& q : p.qs) CHECK(q.k == 0);
    CHECK(!p.narrow && !p.wide);
  }
  ok("k_ignored");
}

void settled() {
  BoolPlan p;
  std::string err;
  CHECK(count_plan(g_img.view(), {Q({{-1, M}, {kBig, S}}),              // a missing MUST term
                                  Q({{kNone, M}, {kBig, S}}),           // a MUST list with no block in the image
                                  Q({{kBig, S}, {kMid, S}, {-1, S}}, 3),   // min_should out of reach
                                  Q({{kBig, M}, {kNone, S}}, 1),        // ... beside a MUST term
                                  Q({{kBig, N}, {kMid, N}}),            // MUST_NOT only
                                  Q({{-1, S}, {kNone, S}}),             // no SHOULD slot left
                                  Q({})},
                   &p, &err) == WSR_OK);
  CHECK(p.qs.empty() && p.roles.empty() && p.items.empty() && p.ev_total == 0);
  // k <= 0 is not settled here
  CHECK(count_plan(g_img.view(), {Q({{kBig, S}}, 0, 0), Q({{-1, M}}), Q({{kMid, M}}, 0, -5)}, &p, &err) == WSR_OK);
  CHECK(p.qs.size() == 2 && p.qs[0].q == 0 && p.qs[1].q == 2);
  CHECK(count_plan(g_img.view(), {}, &p, &err) == WSR_OK && p.qs.empty());
  CHECK(plan_count(g_img.view(), nullptr, 0, false, 4, &p, &err) == WSR_OK);
  ok("settled");
}

void items() {
  BoolPlan c, b;
  std::string err;
  for (uint32_t target : {1u, 4u, 63u})
    for (int shard = 0; shard < 2; ++shard) {
      const ImageView v = shard ? g_img.view(2500, 5000) : g_img.view();
      CHECK(count_plan(v, live(10), &c, &err, target) == WSR_OK);
      CHECK(plan_bool(v, live(10).data(), 5, 10, true, target, &b, &err) == WSR_OK);
      // plan_bool's queries, roles, lead and item ranges; no event slots
      CHECK(same_tables(b, c, false) && !c.items.empty());
      CHECK(b.ev_total > 0 && c.ev_total == 0);
      for (const OrItem& it : c.items) CHECK(it.ev_cap == 0 && it.ev_base == 0 && it.doc_lo < it.doc_hi);
    }
  // (the lead's cut: small has one block, ending at 3100 -- the items past it are dropped)
  CHECK(count_plan(g_img.view(), {Q({{kSmall, M}, {kBig, S}})}, &c, &err) == WSR_OK);
  CHECK(c.qs[0].n_items == 2 && c.items[0].doc_lo == 0 && c.items[0].doc_hi == 3000 && c.items[1].doc_hi == 6000);
  ok("items");
}

void errors() {
  BoolPlan p;
  std::string err;
  const wsr_bool_query good = Q({{kBig, M}, {kMid, S}});
  auto refused = [&](wsr_bool_query bad, int code, const char* msg) {
    err.clear();
    CHECK(count_plan(g_img.view(), {good, bad}, &p, &err) == code);
    CHECK(err == std::string("query 1: ") + msg);
    CHECK(p.qs.empty() && p.items.empty());   // a refused plan holds nothing
  };
  wsr_bool_query b = good;
  b.n_terms = WSR_MAX_OR_TERMS + 1;
  refused(b, WSR_E_LIMIT, "a boolean query has at most WSR_MAX_OR_TERMS terms");
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
  // (k is no error; what lies past n_terms is not read)
  b = good, b.k = WSR_MAX_K + 1, b.role[2] = 9, b.list_ids[2] = 1 << 30;
  CHECK(count_plan(g_img.view(), {good, b}, &p, &err) == WSR_OK && p.qs.size() == 2);
  // null arguments with nq > 0, a negative nq
  CHECK(plan_count(g_img.view(), nullptr, 1, true, 4, &p, &err) == WSR_E_INVALID && err == "bad arguments");
  CHECK(plan_count(g_img.view(), &good, 1, false, 4, &p, &err) == WSR_E_INVALID && err == "bad arguments");
  CHECK(plan_count(g_img.view(), &good, -1, true, 4, &p, &err) == WSR_E_INVALID && err == "bad arguments");
  CHECK(p.qs.empty() && p.items.empty());
  ok("errors");
}

}  // namespace

int main() {
  k_ignored();
  settled();
  items();
  errors();
  return 0;
}
