// CPU check of the wsr_score_docs plan in wiser_amd/csrc/score_plan.cc
// (tests/test_score_plan.py): over a hand-made image directory, the sort is
// the stable one, every item holds at most 64 consecutive sorted candidates of
// one query, every candidate that needs an answer from the device lands in
// exactly one item, the index array is a permutation, and the error returns.
// One "ok <case>" line per case; exit status 0.
#include "../../wiser_amd/csrc/score_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <numeric>
#include <string>
#include <vector>

using namespace wiser;

namespace {

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      std::fprintf(stderr, "score_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                     \
    }                                                                                   \
  } while (0)

void ok(const char* name) { std::printf("ok %s\n", name); }

// The image: lists 0 and 1 have blocks, list 2 has none here (a shard that
// holds no posting of it), 3 lists in all; an index of kDocs docs.
constexpr int64_t kDocs = 5000;
struct Image {
  std::vector<ListDev> lists;
  std::vector<BlockDev> blocks;
  Image() {
    for (uint32_t nblk : {3u, 1u, 0u}) {
      ListDev L{};
      L.blk0 = static_cast<uint32_t>(blocks.size());
      L.nblk = nblk;
      for (uint32_t j = 0; j < nblk; ++j) blocks.push_back(BlockDev{});
      lists.push_back(L);
    }
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

wsr_query Q(std::initializer_list<int32_t> ids, int32_t flags = 0) {
  wsr_query q{};
  q.n_terms = static_cast<int32_t>(ids.size());
  q.k = 0;   // (ignored)
  q.flags = flags;
  int t = 0;
  for (int32_t id : ids) q.list_ids[t++] = id;
  return q;
}

struct Call {
  std::vector<wsr_query> qs;
  std::vector<int64_t> off{0};
  std::vector<int32_t> docs;
  void add(const wsr_query& q, const std::vector<int32_t>& d) {
    qs.push_back(q);
    docs.insert(docs.end(), d.begin(), d.end());
    off.push_back(static_cast<int64_t>(docs.size()));
  }
  int plan(const ImageView& v, ScorePlan* p, std::string* err) const {
    return plan_score_docs(v, kDocs, qs.data(), static_cast<int32_t>(qs.size()), off.data(), docs.data(), p, err);
  }
};

// the properties every plan has; live(i): query i has a term with blocks in the image
void check_plan(const Call& c, const ImageView& v, const ScorePlan& p, const std::vector<bool>& live) {
  const size_t total = c.docs.size();
  CHECK(p.docs.size() == total && p.index.size() == total && p.qs.size() == c.qs.size());
  // the index array is a permutation, and the sorted docs are the caller's through it
  std::vector<uint32_t> seen(total, 0);
  for (size_t j = 0; j < total; ++j) {
    CHECK(p.index[j] < total);
    ++seen[p.index[j]];
    CHECK(p.docs[j] == static_cast<uint32_t>(c.docs[p.index[j]]));
  }
  for (uint32_t s : seen) CHECK(s == 1);
  // per query: its own candidates, ascending, equal ids in the caller's order (stable)
  for (size_t i = 0; i < c.qs.size(); ++i)
    for (int64_t j = c.off[i]; j < c.off[i + 1]; ++j) {
      CHECK(p.index[j] >= c.off[i] && p.index[j] < c.off[i + 1]);
      if (j > c.off[i]) {
        CHECK(p.docs[j - 1] <= p.docs[j]);
        if (p.docs[j - 1] == p.docs[j]) CHECK(p.index[j - 1] < p.index[j]);
      }
    }
  // items: at most kScoreLanes candidates of one query, consecutive; together they cover exactly
  // the candidates of the live queries that lie in the image's doc range, each once
  std::vector<uint32_t> covered(total, 0);
  for (const ScoreItem& it : p.items) {
    CHECK(it.q < c.qs.size() && live[it.q]);
    CHECK(it.n >= 1 && it.n <= kScoreLanes && kScoreLanes == 64);
    CHECK(it.first >= c.off[it.q] && it.first + it.n <= c.off[it.q + 1]);
    for (uint32_t j = it.first; j < it.first + it.n; ++j) ++covered[j];
  }
  for (size_t i = 0; i < c.qs.size(); ++i)
    for (int64_t j = c.off[i]; j < c.off[i + 1]; ++j) {
      const bool in = p.docs[j] >= v.doc_lo && p.docs[j] < v.doc_hi;
      CHECK(covered[j] == ((live[i] && in) ? 1u : 0u));
    }
}

void test_sort_and_items() {
  Call c;
  c.add(Q({0, 1}), {9, 3, 3, 7, 3, 0, 4999, 9});            // duplicates, any order
  c.add(Q({1}), {});                                        // no candidates, between two that have some
  std::vector<int32_t> many(64 * 3 + 1);
  for (size_t j = 0; j < many.size(); ++j) many[j] = static_cast<int32_t>((j * 2654435761u) % kDocs);
  c.add(Q({0, -1, 2}), many);                               // 193 candidates: items of 64, 64, 64, 1
  std::vector<int32_t> rev(64);
  for (int j = 0; j < 64; ++j) rev[j] = 640 - 10 * j;
  c.add(Q({1, 1}), rev);                                    // exactly 64, reversed: one item
  rev.push_back(5);
  c.add(Q({0}), rev);                                       // 65: two items
  c.add(Q({0}), {17});                                      // 1
  c.add(Q({2, -1}), {1, 2, 3});                             // no term has blocks here: no item
  c.add(Q({}), {4, 5});                                     // no terms: no item
  ScorePlan p;
  std::string err;
  CHECK(c.plan(g_img.view(), &p, &err) == WSR_OK);
  const std::vector<bool> live{true, true, true, true, true, true, false, false};
  check_plan(c, g_img.view(), p, live);
  // the first query, spelled out: (doc, place) in stable order
  const uint32_t want_docs[] = {0, 3, 3, 3, 7, 9, 9, 4999}, want_idx[] = {5, 1, 2, 4, 3, 0, 7, 6};
  for (int j = 0; j < 8; ++j) CHECK(p.docs[j] == want_docs[j] && p.index[j] == want_idx[j]);
  std::vector<uint32_t> per_q(c.qs.size(), 0);
  for (const ScoreItem& it : p.items) ++per_q[it.q];
  CHECK((per_q == std::vector<uint32_t>{1, 0, 4, 1, 2, 1, 0, 0}));
  CHECK(p.items[1].q == 2 && p.items[1].n == 64 && p.items[4].n == 1);
  // the resolved terms: a list without blocks in the image counts as missing
  CHECK(p.qs[2].nt == 3 && p.qs[2].list[0] == 0 && p.qs[2].list[1] == -1 && p.qs[2].list[2] == -1);
  CHECK(p.qs[3].nt == 2 && p.qs[3].list[0] == 1 && p.qs[3].list[1] == 1 && p.qs[3].list[2] == -1);
  ok("sort_and_items");
}

void test_shard_range() {
  // an image of docs [100, 300): only the candidates inside it are put into items
  Call c;
  std::vector<int32_t> d;
  for (int j = 0; j < 400; ++j) d.push_back((j * 37) % 400);
  c.add(Q({0}), d);
  c.add(Q({1}), {99, 100, 299, 300, 100});
  c.add(Q({0}), {0, 99, 300, 4999});                        // none in range: no item
  ScorePlan p;
  std::string err;
  const ImageView v = g_img.view(100, 300);
  CHECK(c.plan(v, &p, &err) == WSR_OK);
  check_plan(c, v, p, {true, true, true});
  std::vector<uint32_t> per_q(3, 0), cand(3, 0);
  for (const ScoreItem& it : p.items) {
    ++per_q[it.q];
    cand[it.q] += it.n;
  }
  CHECK((per_q == std::vector<uint32_t>{4, 1, 0}) && (cand == std::vector<uint32_t>{200, 3, 0}));
  ok("shard_range");
}

void test_empty() {
  ScorePlan p;
  std::string err;
  CHECK(plan_score_docs(g_img.view(), kDocs, nullptr, 0, nullptr, nullptr, &p, &err) == WSR_OK);
  CHECK(p.items.empty() && p.docs.empty());
  Call c;
  c.add(Q({0}), {});
  CHECK(c.plan(g_img.view(), &p, &err) == WSR_OK && p.items.empty() && p.qs.size() == 1);
  // a one-term phrase flag is a single-term query; WSR_QUERY_OR changes nothing
  Call d;
  d.add(Q({0}, WSR_QUERY_PHRASE), {1});
  d.add(Q({0, 1}, WSR_QUERY_OR), {1});
  CHECK(d.plan(g_img.view(), &p, &err) == WSR_OK && p.items.size() == 2);
  ok("empty");
}

void test_errors() {
  ScorePlan p;
  auto rc_of = [&](const wsr_query& q, const std::vector<int32_t>& docs, const char* msg) {
    Call c;
    c.add(Q({0}), {1, 2});
    c.add(q, docs);
    std::string err = "unset";
    const int rc = c.plan(g_img.view(), &p, &err);
    if (rc != WSR_OK) CHECK(err.find(msg) != std::string::npos);
    return rc;
  };
  wsr_query q17 = Q({0});
  q17.n_terms = 17;
  CHECK(rc_of(q17, {1}, "query 1: more than WSR_MAX_TERMS") == WSR_E_LIMIT);
  wsr_query q16 = Q({0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1});
  CHECK(rc_of(q16, {1}, "") == WSR_OK);
  CHECK(rc_of(Q({0, 1}, WSR_QUERY_PHRASE), {1}, "phrase") == WSR_E_INVALID);
  CHECK(rc_of(Q({0, 1}, WSR_QUERY_PHRASE | WSR_QUERY_OR), {1}, "phrase") == WSR_E_INVALID);
  CHECK(rc_of(Q({0, 1}, 4), {1}, "unknown flags") == WSR_E_INVALID);
  CHECK(rc_of(Q({0, 1 << 30}), {1}, "list id") == WSR_E_INVALID);
  CHECK(rc_of(Q({0, 3}), {1}, "list id") == WSR_E_INVALID);
  CHECK(rc_of(Q({-2}), {1}, "list id") == WSR_E_INVALID);
  CHECK(rc_of(Q({-1}), {1}, "") == WSR_OK);
  CHECK(rc_of(Q({0}), {1, -1}, "doc id") == WSR_E_INVALID);
  CHECK(rc_of(Q({0}), {static_cast<int32_t>(kDocs)}, "doc id") == WSR_E_INVALID);
  CHECK(rc_of(Q({0}), {static_cast<int32_t>(kDocs) - 1}, "") == WSR_OK);
  // a doc id of a query whose terms are all missing is checked too
  CHECK(rc_of(Q({-1}), {static_cast<int32_t>(kDocs)}, "doc id") == WSR_E_INVALID);
  // doc_off: descending, or not from 0
  const wsr_query qs[2] = {Q({0}), Q({1})};
  const int32_t docs[4] = {1, 2, 3, 4};
  std::string err;
  const int64_t desc[3] = {0, 3, 2}, from1[3] = {1, 2, 4}, fine[3] = {0, 2, 4};
  CHECK(plan_score_docs(g_img.view(), kDocs, qs, 2, desc, docs, &p, &err) == WSR_E_INVALID);
  CHECK(err.find("ascending") != std::string::npos);
  CHECK(plan_score_docs(g_img.view(), kDocs, qs, 2, from1, docs, &p, &err) == WSR_E_INVALID);
  CHECK(plan_score_docs(g_img.view(), kDocs, qs, 2, fine, docs, &p, &err) == WSR_OK);
  CHECK(plan_score_docs(g_img.view(), kDocs, qs, 2, nullptr, docs, &p, &err) == WSR_E_INVALID);
  CHECK(plan_score_docs(g_img.view(), kDocs, qs, 2, fine, nullptr, &p, &err) == WSR_E_INVALID);
  CHECK(plan_score_docs(g_img.view(), kDocs, qs, -1, fine, docs, &p, &err) == WSR_E_INVALID);
  ok("errors");
}

}  // namespace

int main() {
  test_sort_and_items();
  test_shard_range();
  test_empty();
  test_errors();
  return 0;
}
