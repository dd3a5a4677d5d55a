// The host's plan of a wsr_search_bool or wsr_count_bool call (bool_plan.h).
#include "bool_plan.h"

#include <algorithm>

#include "or_plan.h"

namespace wiser {

namespace {
int fail(std::string* err, int code, const std::string& msg) {
  *err = msg;
  return code;
}

// check_bool_query's rule; counting: k is not looked at (wsr_count_bool)
int check_query(const ImageView& v, const wsr_bool_query& q, bool counting, std::string* err) {
  if (q.n_terms > WSR_MAX_OR_TERMS) return fail(err, WSR_E_LIMIT, "a boolean query has at most WSR_MAX_OR_TERMS terms");
  if (!counting && q.k > WSR_MAX_K) return fail(err, WSR_E_LIMIT, "k over WSR_MAX_K");
  if (q.n_terms < 0) return fail(err, WSR_E_INVALID, "n_terms is negative");
  if (q.min_should < 0) return fail(err, WSR_E_INVALID, "min_should is negative");
  const int32_t n_lists = static_cast<int32_t>(v.n_lists);
  for (int t = 0; t < q.n_terms; ++t) {
    if (q.role[t] > WSR_ROLE_MUST_NOT) return fail(err, WSR_E_INVALID, "a term's role is none of WSR_ROLE_*");
    if (q.list_ids[t] < -1 || q.list_ids[t] >= n_lists) return fail(err, WSR_E_INVALID, "list id out of range");
  }
  return WSR_OK;
}

// plan_bool, or (counting) plan_count: no k anywhere and no event slots
int plan(const ImageView& v, const wsr_bool_query* q, int32_t nq, int32_t stride, bool have_out, uint32_t target,
         bool counting, BoolPlan* out, std::string* err) {
  BoolPlan& p = *out;
  p.qs.clear();
  p.roles.clear();
  p.items.clear();
  p.ev_total = 0;
  p.nt_max = 0;
  p.narrow = p.wide = false;
  if (nq < 0 || (nq > 0 && (!q || !have_out))) return fail(err, WSR_E_INVALID, "bad arguments");
  for (int i = 0; i < nq; ++i) {
    auto at = [i] { return "query " + std::to_string(i) + ": "; };
    if (!counting && q[i].k > stride) return fail(err, WSR_E_LIMIT, at() + "k over the call's hit stride");
    std::string why;
    const int rc = check_query(v, q[i], counting, &why);
    if (rc) return fail(err, rc, at() + why);
  }
  for (int i = 0; i < nq; ++i) {
    const wsr_bool_query& s = q[i];
    if ((!counting && s.k <= 0) || s.n_terms == 0) continue;
    OrQuery oq{};
    BoolRoles r{};
    oq.q = i;
    oq.k = counting ? 0 : s.k;
    bool has_must = false, settled = false;
    for (int t = 0; t < s.n_terms; ++t) {
      const int32_t id = s.list_ids[t];
      const bool holds = id >= 0 && v.lists[id].nblk > 0;   // (no blocks: none in this image)
      if (s.role[t] == WSR_ROLE_MUST) {
        has_must = true;
        if (!holds) settled = true;
      }
      if (!holds) continue;
      const uint32_t bit = 1u << oq.nt;
      (s.role[t] == WSR_ROLE_MUST ? r.must_mask : s.role[t] == WSR_ROLE_SHOULD ? r.should_mask : r.not_mask) |= bit;
      oq.list[oq.nt++] = id;
    }
    r.need_should = static_cast<uint32_t>(std::max(s.min_should, has_must ? 0 : 1));
    if (settled || static_cast<uint32_t>(__builtin_popcount(r.should_mask)) < r.need_should) continue;
    r.lead = -1;
    for (int t = 0; t < oq.nt; ++t)
      if (((r.must_mask >> t) & 1u) &&
          (r.lead < 0 || v.lists[oq.list[t]].nblk < v.lists[oq.list[r.lead]].nblk))
        r.lead = t;
    const size_t item0 = p.items.size();
    const uint64_t ev0 = p.ev_total;
    // (the cut is over all kept slots, MUST_NOT lists included: their blocks are read too; the
    // MaxScore bounds are over the scoring slots alone)
    plan_or_query(v, target, &oq, &p.items, &p.ev_total, ~r.not_mask);
    if (r.lead >= 0) {
      // a matching doc is a posting of the lead list
      const ListDev& L = v.lists[oq.list[r.lead]];
      size_t w = item0;
      uint64_t ev = ev0;
      for (size_t j = item0; j < p.items.size(); ++j) {
        OrItem it = p.items[j];
        const uint64_t nb = blocks_overlapping(v, L, it.doc_lo, it.doc_hi);
        if (!nb) continue;
        it.ev_cap = static_cast<uint32_t>(std::min<uint64_t>(it.ev_cap, 128 * nb));
        it.ev_base = ev;
        ev += it.ev_cap;
        p.items[w++] = it;
      }
      p.items.resize(w);
      p.ev_total = ev;
      oq.n_items = static_cast<uint32_t>(w - item0);
    }
    if (!oq.n_items) continue;
    for (uint32_t j = 0; j < oq.n_items; ++j) p.items[oq.item_base + j].oq = static_cast<uint32_t>(p.qs.size());
    p.nt_max = std::max(p.nt_max, oq.nt);
    if (!counting) (oq.k > kMaxK ? p.wide : p.narrow) = true;
    p.qs.push_back(oq);
    p.roles.push_back(r);
  }
  if (counting) {
    for (OrItem& it : p.items) it.ev_cap = 0, it.ev_base = 0;
    p.ev_total = 0;
  }
  return WSR_OK;
}
}  // namespace

int check_bool_query(const ImageView& v, const wsr_bool_query& q, std::string* err) {
  return check_query(v, q, false, err);
}

int plan_bool(const ImageView& v, const wsr_bool_query* q, int32_t nq, int32_t stride, bool have_out,
              uint32_t target, BoolPlan* out, std::string* err) {
  return plan(v, q, nq, stride, have_out, target, false, out, err);
}

int plan_count(const ImageView& v, const wsr_bool_query* q, int32_t nq, bool have_out, uint32_t target,
               BoolPlan* out, std::string* err) {
  return plan(v, q, nq, 0, have_out, target, true, out, err);
}

}  // namespace wiser
