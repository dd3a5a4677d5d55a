// CPU check of the tiny class in the upload plan (tests/test_tiny_plan.py):
// plan_upload's tiny count and the general grid that is left, over a hand-made
// image directory, against is_tiny_query applied query by query; and what
// launches_of makes of them.  One "ok <case>" line per case; exit status 0.
#include "../../wiser_amd/csrc/batch_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

using namespace wiser;

namespace {

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "tiny_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

// list id -> blocks here, a decoded tail, a bitmap
//   0: none   1: 1 block, tail   2: 1 block, tail   3: 1 block, a full pack (no tail)
//   4: 2 blocks, tail   5: 1 block, tail, bitmap   6: 40 blocks, bitmap   7: 3 blocks, no tail
enum { kNone = 0, kTailA, kTailB, kPack, kTwo, kTailBm, kLong, kThree, kLists };

struct Image {
  std::vector<ListDev> lists;
  std::vector<uint64_t> bytes;
  void add(uint32_t nblk, bool tail, bool bm) {
    ListDev L{};
    L.nblk = nblk;
    L.tail = tail ? 256 * lists.size() : kNoTail;
    L.tail_cnt = tail ? 100 : 128;
    L.bm = bm ? 64 * lists.size() : kNoDense;
    L.idf = 1.0;
    bytes.push_back(100);
    lists.push_back(L);
  }
  Image() {
    add(0, false, false);
    add(1, true, false);
    add(1, true, false);
    add(1, false, false);
    add(2, true, false);
    add(1, true, true);
    add(40, false, true);
    add(3, false, false);
    CHECK(lists.size() == kLists);
  }
  ImageView view() const {
    ImageView v;
    v.lists = lists.data();
    v.n_lists = lists.size();
    v.list_bytes = bytes.data();
    v.pos_bytes = bytes.data();
    v.dense_ratio = 1.0f;
    v.doc_hi = 10000;
    v.positions = true;
    v.lean_wgs = v.lean_wgs_two = v.lean_wgs_ph = 100;
    v.gen_cap = 40;
    return v;
  }
};
const Image g_img;

wsr_query Q(std::initializer_list<int32_t> ids, int32_t k, int32_t flags = 0) {
  wsr_query q{};
  q.n_terms = static_cast<int32_t>(ids.size());
  q.k = k;
  q.flags = flags;
  int t = 0;
  for (int32_t id : ids) q.list_ids[t++] = id;
  return q;
}

BatchClass cls(const std::vector<wsr_query>& qs) {
  UploadPlan p;
  std::string err;
  CHECK(plan_upload(g_img.view(), qs.data(), static_cast<int32_t>(qs.size()), WSR_MAX_K, kSegCost, &p, &err) ==
        WSR_OK);
  return p.cls;
}

// the rule, query by query, from the image alone
bool rule(const wsr_query& q) {
  if (q.n_terms != 2 || q.k <= 0) return false;
  for (int t = 0; t < 2; ++t)
    if (q.list_ids[t] < 0 || q.list_ids[t] >= kLists || g_img.lists[q.list_ids[t]].nblk == 0) return false;
  const ListDev &a = g_img.lists[q.list_ids[0]], &b = g_img.lists[q.list_ids[1]];
  return is_tiny_query(q.n_terms, (q.flags & WSR_QUERY_PHRASE) ? kQueryPhrase : 0, q.k,
                       is_tiny_list(a.nblk, a.tail), is_tiny_list(b.nblk, b.tail));
}

void rule_case() {
  CHECK(is_tiny_list(1, 0) && !is_tiny_list(1, kNoTail) && !is_tiny_list(2, 0) && !is_tiny_list(0, 0));
  CHECK(is_tiny_query(2, 0, kMaxK, true, true) && !is_tiny_query(2, 0, kMaxK + 1, true, true));
  CHECK(!is_tiny_query(2, kQueryPhrase, 10, true, true) && !is_tiny_query(3, 0, 10, true, true));
  CHECK(!is_tiny_query(1, 0, 10, true, true) && !is_tiny_query(2, 0, 10, false, true) &&
        !is_tiny_query(2, 0, 10, true, false));
  std::printf("ok rule\n");
}

void count_case() {
  const int32_t PH = WSR_QUERY_PHRASE;
  const std::vector<wsr_query> qs = {
      Q({kTailA, kTailB}, 10),      Q({kTailB, kTailA}, kMaxK), Q({kTailA, kTailA}, 1),  Q({kTailA, kTailBm}, 10),
      Q({kTailBm, kTailBm}, 10),    Q({kTailA, kTailB}, kMaxK + 1), Q({kTailA, kTailB}, 10, PH), Q({kTailA, kPack}, 10),
      Q({kPack, kTailA}, 10),       Q({kTailA, kTwo}, 10),      Q({kTailA, kNone}, 10),  Q({kTailA, -1}, 10),
      Q({kTailA, kTailB}, 0),       Q({kTailA}, 10),            Q({kTailA, kTailB, kTailBm}, 10), Q({kTailA, kLong}, 10),
      Q({kThree, kTwo}, 10)};
  int want = 0;
  std::vector<bool> each;
  for (const wsr_query& q : qs) {
    const bool t = rule(q);
    each.push_back(t);
    want += t;
  }
  CHECK(want == 5);
  CHECK(each[0] && each[1] && each[2] && each[3] && each[4]);
  const BatchClass c = cls(qs);
  CHECK(c.n_tiny == want);
  // one query at a time: the count is the rule's answer
  for (size_t i = 0; i < qs.size(); ++i) CHECK(cls({qs[i]}).n_tiny == (each[i] ? 1 : 0));
  std::printf("ok count\n");
}

void grids_case() {
  // the general need without the tiny queries: {1,3} 1 block, {7,4} 2 blocks; {1,2} and {2,1} are tiny
  BatchClass c = cls({Q({kTailA, kTailB}, 10), Q({kTailB, kTailA}, 10), Q({kTailA, kPack}, 10), Q({kThree, kTwo}, 10)});
  CHECK(c.n_tiny == 2 && c.has_gen && c.seg_grid == 5 && c.seg_grid_rest == 3);
  // only tiny queries: the grid of an empty class is 1
  c = cls({Q({kTailA, kTailB}, 10), Q({kTailB, kTailA}, 10)});
  CHECK(c.n_tiny == 2 && c.has_gen && c.seg_grid == 2 && c.seg_grid_rest == 1);
  // a tiny query whose other list has a bitmap is lean by the other rule: no general need either way
  c = cls({Q({kTailA, kTailBm}, 10)});
  CHECK(c.n_tiny == 1 && !c.has_gen && c.has_conj_lean && c.seg_grid == 1 && c.seg_grid_rest == 1);
  c = cls({Q({kTailA, kLong}, 10)});
  CHECK(c.n_tiny == 0 && c.seg_grid_rest == c.seg_grid);
  std::printf("ok grids\n");
}

void launches_case() {
  BatchClass c = cls({Q({kTailA, kTailB}, 10), Q({kTailA, kPack}, 10), Q({kThree, kTwo}, 10)});
  CHECK(c.n_tiny == 1 && c.seg_grid == 4 && c.seg_grid_rest == 3);
  Launches l = launches_of(c, false, false);
  CHECK(l.tiny && l.tiny_class && l.gen && l.conj && l.gen_grid == 3);
  // a shard step and a carried owner replay have no tiny class
  l = launches_of(c, true, false);
  CHECK(!l.tiny && !l.tiny_class && l.gen && l.gen_grid == 4);
  l = launches_of(c, false, true);
  CHECK(!l.tiny && !l.tiny_class && l.gen && l.gen_grid == 4);
  // no tiny query: as before
  c = cls({Q({kTailA, kPack}, 10)});
  l = launches_of(c, false, false);
  // no launch, but the class stays on: a tiny query the device finds is flagged
  CHECK(!l.tiny && l.tiny_class && l.gen_grid == c.seg_grid && c.seg_grid_rest == c.seg_grid);
  const BatchClass fresh;
  CHECK(!launches_of(fresh, false, false).tiny && launches_of(fresh, false, false).gen_grid == fresh.seg_grid);
  std::printf("ok launches_of\n");
}

}  // namespace

int main() {
  rule_case();
  count_case();
  grids_case();
  launches_case();
  return 0;
}
