// The host's plan of a wsr_score_docs call (score_plan.h).
#include "score_plan.h"

#include <algorithm>

namespace wiser {

namespace {
int fail(std::string* err, int code, const std::string& msg) {
  *err = msg;
  return code;
}
}  // namespace

int plan_score_docs(const ImageView& v, int64_t n_docs, const wsr_query* q, int32_t nq, const int64_t* doc_off,
                    const int32_t* docs, ScorePlan* out, std::string* err) {
  ScorePlan& p = *out;
  p.qs.clear();
  p.items.clear();
  p.docs.clear();
  p.index.clear();
  if (nq < 0 || (nq > 0 && (!q || !doc_off))) return fail(err, WSR_E_INVALID, "bad arguments");
  if (nq == 0) return WSR_OK;
  if (doc_off[0] != 0) return fail(err, WSR_E_INVALID, "doc_off[0] is not 0");
  for (int i = 0; i < nq; ++i)
    if (doc_off[i + 1] < doc_off[i]) return fail(err, WSR_E_INVALID, "doc_off is not ascending");
  const int64_t total = doc_off[nq];
  if (total >= kScoreMaxPairs) return fail(err, WSR_E_LIMIT, "over 2^31 candidates in one call");
  if (total > 0 && !docs) return fail(err, WSR_E_INVALID, "bad arguments");
  const int32_t n_lists = static_cast<int32_t>(v.n_lists);
  p.qs.resize(nq);
  for (int i = 0; i < nq; ++i) {
    const wsr_query& s = q[i];
    auto at = [i] { return "query " + std::to_string(i) + ": "; };
    if (s.n_terms > WSR_MAX_TERMS) return fail(err, WSR_E_LIMIT, at() + "more than WSR_MAX_TERMS terms");
    if (s.flags & ~(WSR_QUERY_PHRASE | WSR_QUERY_OR)) return fail(err, WSR_E_INVALID, at() + "unknown flags");
    if (is_phrase_query(s.n_terms, (s.flags & WSR_QUERY_PHRASE) ? kQueryPhrase : 0))
      return fail(err, WSR_E_INVALID, at() + "a phrase query: positions are not checked here");
    ScoreQuery& d = p.qs[i];
    d.nt = s.n_terms < 0 ? 0 : s.n_terms;
    for (int t = 0; t < kMaxTerms; ++t) {
      d.list[t] = -1;
      if (t >= d.nt) continue;
      const int32_t id = s.list_ids[t];
      if (id < -1 || id >= n_lists) return fail(err, WSR_E_INVALID, at() + "list id out of range");
      if (id >= 0 && v.lists[id].nblk > 0) d.list[t] = id;   // (no blocks: none in this image)
    }
  }
  for (int64_t j = 0; j < total; ++j)
    if (docs[j] < 0 || docs[j] >= n_docs) return fail(err, WSR_E_INVALID, "doc id outside the index");

  p.docs.resize(static_cast<size_t>(total));
  p.index.resize(static_cast<size_t>(total));
  std::vector<uint64_t> keys;   // doc id << 32 | place: the place breaks ties, so the order is the stable one
  for (int i = 0; i < nq; ++i) {
    const int64_t lo = doc_off[i], hi = doc_off[i + 1];
    keys.resize(static_cast<size_t>(hi - lo));
    for (int64_t j = lo; j < hi; ++j)
      keys[j - lo] = (static_cast<uint64_t>(static_cast<uint32_t>(docs[j])) << 32) | static_cast<uint32_t>(j);
    std::sort(keys.begin(), keys.end());
    for (int64_t j = lo; j < hi; ++j) {
      p.docs[j] = static_cast<uint32_t>(keys[j - lo] >> 32);
      p.index[j] = static_cast<uint32_t>(keys[j - lo]);
    }
    const ScoreQuery& d = p.qs[i];
    if (std::all_of(d.list, d.list + kMaxTerms, [](int32_t id) { return id < 0; })) continue;
    // the candidates inside the image's doc range are consecutive in the sorted order
    const uint32_t* b = p.docs.data();
    const int64_t f = std::lower_bound(b + lo, b + hi, v.doc_lo) - b;
    const int64_t e = std::lower_bound(b + f, b + hi, v.doc_hi) - b;
    for (int64_t c = f; c < e; c += kScoreLanes) {
      ScoreItem it;
      it.q = static_cast<uint32_t>(i);
      it.first = static_cast<uint32_t>(c);
      it.n = static_cast<uint32_t>(std::min<int64_t>(kScoreLanes, e - c));
      p.items.push_back(it);
    }
  }
  return WSR_OK;
}

}  // namespace wiser
