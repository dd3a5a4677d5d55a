// The host's plan of a batch upload (batch_plan.h).
#include "batch_plan.h"

#include <algorithm>

#include "or_plan.h"

namespace wiser {

std::vector<int32_t> query_terms(const wsr_query& q) {
  std::vector<int32_t> t(q.n_terms > 0 ? static_cast<size_t>(q.n_terms) : 0u);
  for (int i = 0; i < q.n_terms; ++i) t[i] = i < WSR_MAX_TERMS ? q.list_ids[i] : q.more_ids[i - WSR_MAX_TERMS];
  return t;
}

namespace {

int fail(std::string* err, int code, const std::string& msg) {
  *err = msg;
  return code;
}

}  // namespace

int check_query(const ImageView& v, const wsr_query& q, std::string* err) {
  if (q.n_terms > WSR_MAX_QUERY_TERMS || q.k > WSR_MAX_K)
    return fail(err, WSR_E_LIMIT, "n_terms or k over the limit");
  if (q.flags & ~(WSR_QUERY_PHRASE | WSR_QUERY_OR)) return fail(err, WSR_E_INVALID, "unknown flags");
  if ((q.flags & WSR_QUERY_OR) && (q.flags & WSR_QUERY_PHRASE))
    return fail(err, WSR_E_INVALID, "a query is a phrase or a disjunction, not both");
  if ((q.flags & WSR_QUERY_OR) && q.n_terms > WSR_MAX_OR_TERMS)
    return fail(err, WSR_E_LIMIT, "a disjunctive query has at most WSR_MAX_OR_TERMS terms");
  if (q.n_terms > WSR_MAX_TERMS && !q.more_ids)
    return fail(err, WSR_E_INVALID, "a query of more than WSR_MAX_TERMS terms needs more_ids");
  if ((q.flags & WSR_QUERY_PHRASE) && q.n_terms > WSR_MAX_PHRASE_TERMS)
    return fail(err, WSR_E_LIMIT, "a phrase query has at most WSR_MAX_PHRASE_TERMS terms");
  if ((q.flags & WSR_QUERY_PHRASE) && q.n_terms > 1 && !v.positions)
    return fail(err, WSR_E_INVALID, "phrase query on an engine opened without positions");
  return WSR_OK;
}

int plan_upload(const ImageView& v, const wsr_query* q, int32_t nq, int32_t stride, uint32_t seg_cap,
                UploadPlan* out, std::string* err) {
  UploadPlan& p = *out;
  p.in.clear();
  p.in.resize(nq);
  p.ext.clear();
  p.orq.clear();
  p.or_items.clear();
  p.or_ev = p.ev_need = p.items_need = 0;
  BatchClass c;
  c.two_conj = c.two_ph = c.one_conj = true;   // (every ...: until a query says otherwise)
  // blocks of the driver lists per class: what the three persistent grids can have to run
  uint64_t lean_need = 0, lean_need_ph = 0, gen_need = 0, gen_need_rest = 0;
  const int32_t n_lists = static_cast<int32_t>(v.n_lists);
  std::vector<int32_t> ids;
  for (int i = 0; i < nq; ++i) {
    const wsr_query& s = q[i];
    auto at = [i] { return "query " + std::to_string(i) + ": "; };
    if (s.k > stride) return fail(err, WSR_E_LIMIT, at() + "k over the batch's hit stride");
    std::string why;
    const int qrc = check_query(v, s, &why);
    if (qrc) return fail(err, qrc, at() + why);
    QueryIn& d = p.in[i];
    d.k = s.k < 0 ? 0 : s.k;
    d.ext = 0;
    if (s.flags & WSR_QUERY_OR) {
      // a disjunctive query: an empty one to the conjunctive plan and kernels
      // (neutral to the batch's class flags), planned here into its own table
      d.n_terms = 0;
      d.flags = 0;
      for (int t = 0; t < kMaxTerms; ++t) d.list[t] = -1;
      c.has_or = true;
      // (only -1 means a missing term; n_terms <= WSR_MAX_OR_TERMS: the ids are inline)
      for (int t = 0; t < s.n_terms; ++t)
        if (s.list_ids[t] < -1 || s.list_ids[t] >= n_lists)
          return fail(err, WSR_E_INVALID, at() + "list id out of range");
      if (s.k <= 0) continue;
      OrQuery oq{};
      oq.q = i;
      oq.k = s.k;
      for (int t = 0; t < s.n_terms; ++t) {
        const int32_t id = s.list_ids[t];
        if (id >= 0 && v.lists[id].nblk > 0) oq.list[oq.nt++] = id;   // (no blocks: none in this image)
      }
      if (oq.nt == 0) continue;
      plan_or_query(v, seg_cap, &oq, &p.or_items, &p.or_ev);
      for (int t = 0; t < oq.nt; ++t) c.algo_static += v.list_bytes[oq.list[t]];
      c.algo_static += 12ull * oq.k;
      for (uint32_t r = 0; r < oq.n_items; ++r)
        p.or_items[oq.item_base + r].oq = static_cast<uint32_t>(p.orq.size());
      if (oq.n_items) {
        c.or_nt_max = std::max(c.or_nt_max, oq.nt);
        (oq.k > kMaxK ? c.or_wide : c.or_narrow) = true;
        p.orq.push_back(oq);
      }
      continue;
    }
    d.n_terms = s.n_terms < 0 ? 0 : s.n_terms;
    const bool phrase = is_phrase_query(s.n_terms, (s.flags & WSR_QUERY_PHRASE) ? kQueryPhrase : 0);
    d.flags = phrase ? kQueryPhrase : 0;
    c.has_phrase = c.has_phrase || phrase;
    c.has_wide = c.has_wide || s.k > kMaxK;
    if (phrase) c.two_ph = c.two_ph && s.k <= kMaxK;
    else {
      c.two_conj = c.two_conj && s.k <= kMaxK && (s.n_terms == 2 || s.n_terms <= 0 || s.k <= 0);
      c.one_conj = c.one_conj && (s.n_terms == 1 || s.n_terms <= 0 || s.k <= 0);
    }
    ids = query_terms(s);
    for (int t = 0; t < kMaxTerms; ++t) d.list[t] = t < d.n_terms ? ids[t] : -1;
    if (d.n_terms > kMaxTerms) {
      d.ext = static_cast<uint32_t>((sizeof(QueryIn) * static_cast<size_t>(nq)) / sizeof(int32_t) + p.ext.size());
      p.ext.insert(p.ext.end(), ids.begin(), ids.end());
    }
    uint32_t nbmin = 0xFFFFFFFFu;
    bool ok = d.n_terms > 0 && d.k > 0;
    for (int t = 0; t < d.n_terms; ++t) {
      const int32_t id = ids[t];
      if (id < 0 || id >= n_lists) { ok = false; continue; }
      nbmin = std::min(nbmin, v.lists[id].nblk);
    }
    if (!ok || nbmin == 0) continue;   // an empty result: no item, no event
    // (a single-term item spans up to kSingleWindows items' blocks)
    const uint64_t seg_max = d.n_terms == 1 ? std::min<uint64_t>(nbmin, uint64_t{kSegCost} * kSingleWindows)
                                            : uint64_t{kSegCost};
    p.ev_need += (static_cast<uint64_t>(nbmin) + seg_max) * 128;
    p.items_need += nbmin;
    // the device's class rule (plan_query_kernel): the driver's blocks are
    // work of the lean conjunctive, the lean phrase or the general grid
    int drv = 0;
    for (int t = 1; t < d.n_terms; ++t)
      if (v.lists[ids[t]].nblk < v.lists[ids[drv]].nblk) drv = t;
    bool others_by_bitmap = true;
    for (int t = 0; t < d.n_terms; ++t) {
      const ListDev& L = v.lists[ids[t]];
      if (t != drv && !probe_by_bitmap(v, L.bm != kNoDense, L.nblk, nbmin)) others_by_bitmap = false;
    }
    const bool lean = is_lean_query(others_by_bitmap, d.n_terms, d.flags);
    (lean ? (phrase ? lean_need_ph : lean_need) : gen_need) += nbmin;
    // the tiny class of a plain run (the device's rule: it comes first there)
    const bool tiny = d.n_terms == 2 &&
                      is_tiny_query(d.n_terms, d.flags, d.k, is_tiny_list(v.lists[ids[0]].nblk, v.lists[ids[0]].tail),
                                    is_tiny_list(v.lists[ids[1]].nblk, v.lists[ids[1]].tail));
    if (tiny) ++c.n_tiny;
    else if (!lean) gen_need_rest += nbmin;
    c.gen_phrase = c.gen_phrase || (phrase && !lean);
    // every term's docid+tf span, and for a phrase query also its
    // position box (the bags the position check reads from)
    for (int t = 0; t < d.n_terms; ++t) {
      c.algo_static += v.list_bytes[ids[t]];
      if (phrase && v.pos_bytes) c.algo_static += v.pos_bytes[ids[t]];
    }
    c.algo_static += 12ull * d.k;
  }
  p.q_bytes = sizeof(QueryIn) * static_cast<size_t>(nq) + sizeof(int32_t) * p.ext.size();
  c.has_conj_lean = lean_need > 0;
  c.has_gen = gen_need > 0;
  c.one_conj = c.one_conj && !c.two_conj;   // (a batch of empty queries only: the two-term instance)
  // persistent grid: never more workgroups than work items can exist
  // (at least one worker each: a grid also drains items the estimate missed)
  auto grid = [](int cap, uint64_t need) {
    return static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(cap, need)));
  };
  c.seg_grid = grid(v.gen_cap, gen_need);
  c.seg_grid_rest = grid(v.gen_cap, gen_need_rest);
  c.lean_wgs = grid(c.two_conj ? v.lean_wgs_two : v.lean_wgs, (lean_need + kLeanWaves - 1) / kLeanWaves);
  c.lean_wgs_ph = grid(v.lean_wgs_ph, (lean_need_ph + kLeanWaves - 1) / kLeanWaves);
  c.n_or = static_cast<int>(p.orq.size());
  c.or_items = static_cast<uint32_t>(p.or_items.size());
  p.cls = c;
  return WSR_OK;
}

}  // namespace wiser
