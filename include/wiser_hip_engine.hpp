// wiser_hip_engine.hpp -- C++ host class above the C ABI (wiser_hip.h) that
// keeps the reference's operator surface:
//   SearchEngineServiceNew::{Load, Search, TermCount, PostinglistSizes}
//   (src/qq_mem/src/engine_services.h:14-27, vacuum_engine.h:119-258)
//   SearchQuery / SearchResultEntry / SearchResult (types.h:205-346)
// Header-only; link libwiser_hip.so.  Errors: the reference aborts (LOG(FATAL))
// on corrupt data; this class throws std::runtime_error instead, and keeps the
// reference's empty-result rules (n_results == 0, any missing term).
#ifndef WISER_HIP_ENGINE_HPP
#define WISER_HIP_ENGINE_HPP

#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "wiser_hip.h"

namespace wiser_hip {

typedef std::vector<std::string> TermList;

struct SearchQuery {  // types.h:205-256
  SearchQuery() {}
  explicit SearchQuery(const TermList& t) : terms(t) {}
  SearchQuery(const TermList& t, bool snippets) : terms(t), return_snippets(snippets) {}
  TermList terms;
  int n_results = 5;
  bool return_snippets = false;  // entries get snippets (host stage, wsr_snippet)
  int n_snippet_passages = 3;
  bool is_phrase = false;        // >= 2 terms: consecutive positions required (WSR_QUERY_PHRASE)
  bool match_any = false;        // disjunctive (WSR_QUERY_OR): the docs that hold any of the terms; a
                                 // missing term contributes nothing (doc_freq 0); not with is_phrase
                                 // or return_snippets
};

struct SearchResultEntry {  // types.h:259-274
  std::string snippet;
  int doc_id = 0;
  double doc_score = 0;
};

struct SearchResult {  // types.h:297-346
  std::vector<SearchResultEntry> entries;
  std::vector<int> doc_freqs;
  std::size_t Size() const { return entries.size(); }
  const SearchResultEntry& operator[](int i) const { return entries[i]; }
};

struct DocScore {  // what a query gives one doc (ScoreDocs; beyond the reference)
  double score = 0;
  uint32_t mask = 0;   // bit t: term t is in the index and its list holds the doc
};

enum class Role { kShould = WSR_ROLE_SHOULD, kMust = WSR_ROLE_MUST, kMustNot = WSR_ROLE_MUST_NOT };

struct BoolQuery {  // wsr_bool_query by term strings (SearchBool; beyond the reference)
  std::vector<std::pair<std::string, Role>> terms;   // in query order, at most WSR_MAX_OR_TERMS
  int n_results = 10;
  int min_should = 0;   // SHOULD terms a doc has to hold at least (1 when no term is MUST)
};

inline void check(int rc) {
  if (rc != WSR_OK) throw std::runtime_error(std::string("wiser_hip: ") + wsr_last_error());
}

// A set of doc ids of the whole index resident on the device (wsr_docset;
// VacuumHipEngine::MakeDocSet): the filter of SearchBool and CountBool.
// Immutable; destroy it before its engine.
class DocSet {
 public:
  DocSet(wsr_handle* h, wsr_docset* s) : h_(h), s_(s) {}
  DocSet(DocSet&& o) noexcept : h_(o.h_), s_(o.s_) { o.s_ = nullptr; }
  DocSet& operator=(DocSet&& o) noexcept {
    if (this != &o) {
      wsr_docset_destroy(h_, s_);
      h_ = o.h_;
      s_ = o.s_;
      o.s_ = nullptr;
    }
    return *this;
  }
  DocSet(const DocSet&) = delete;
  DocSet& operator=(const DocSet&) = delete;
  ~DocSet() { wsr_docset_destroy(h_, s_); }

  const wsr_docset* get() const { return s_; }
  int64_t Count() const {
    int64_t n = 0;
    check(wsr_docset_count(h_, s_, &n));
    return n;
  }
  std::vector<int32_t> Ids() const {   // ascending
    std::vector<int32_t> out(static_cast<size_t>(Count()));
    int64_t n = 0;
    check(wsr_docset_ids(h_, s_, out.data(), static_cast<int64_t>(out.size()), &n));
    return out;
  }

 private:
  wsr_handle* h_;
  wsr_docset* s_;
};

class VacuumHipEngine {
 public:
  // bloom_enable_factor: CreateSearchEngine's (engine_factory.h:33-34), default 1
  explicit VacuumHipEngine(const std::string& dir, int device = 0, int bloom_enable_factor = 1)
      : dir_(dir), device_(device), bloom_factor_(bloom_enable_factor) {}
  ~VacuumHipEngine() { wsr_close(h_); }
  VacuumHipEngine(const VacuumHipEngine&) = delete;
  VacuumHipEngine& operator=(const VacuumHipEngine&) = delete;

  void Load() {
    if (h_) throw std::runtime_error("Engine is already loaded.");
    wsr_open_opts o{device_, 0, 0, 0, 1, bloom_factor_};   // positions: phrase queries served
    check(wsr_open(dir_.c_str(), &o, &h_));
  }

  int TermCount() const {
    int32_t n = 0;
    check(wsr_term_count(h_, &n));
    return n;
  }

  std::map<std::string, int> PostinglistSizes(const TermList& terms) const {
    std::map<std::string, int> out;
    for (const auto& t : terms) {
      int32_t id, df;
      check(wsr_lookup(h_, t.c_str(), &id, &df));
      if (id >= 0) out[t] = df;
    }
    return out;
  }

  SearchResult Search(const SearchQuery& q) { return SearchBatch({q})[0]; }

  // VacuumEngine::GenerateSnippet (vacuum_engine.h:286-296) for a result entry
  std::string Snippet(const wsr_query& q, int doc_id, int n_passages) const {
    std::string s(4096, '\0');
    int32_t n = 0;
    check(wsr_snippet(h_, &q, doc_id, n_passages, &s[0], static_cast<int32_t>(s.size()), &n));
    if (n > static_cast<int32_t>(s.size())) {
      s.assign(n, '\0');
      check(wsr_snippet(h_, &q, doc_id, n_passages, &s[0], n, &n));
    }
    s.resize(n);
    return s;
  }

  // wsr_score_docs: per query, what it gives each of its doc ids, in the
  // caller's order.  mask bit t: term t is in the index and its list holds the
  // doc; score: the sum of those terms' BM25 in query order from 0.0 (a full
  // mask: the conjunctive score; any mask: the match_any score).  n_results is
  // ignored; the engine checks the term limit (WSR_MAX_TERMS) and refuses a
  // phrase of two or more terms.
  std::vector<std::vector<DocScore>> ScoreDocsBatch(const std::vector<SearchQuery>& qs,
                                                    const std::vector<std::vector<int>>& doc_ids) {
    if (qs.size() != doc_ids.size()) throw std::runtime_error("wiser_hip: one doc id list per query");
    std::vector<wsr_query> in(qs.size());
    std::vector<int64_t> off(qs.size() + 1, 0);
    std::vector<int32_t> docs;
    for (size_t i = 0; i < qs.size(); ++i) {
      const SearchQuery& q = qs[i];
      wsr_query& w = in[i];
      w = wsr_query{};
      w.n_terms = static_cast<int32_t>(q.terms.size());
      w.flags = ((q.is_phrase && q.terms.size() > 1) ? WSR_QUERY_PHRASE : 0) | (q.match_any ? WSR_QUERY_OR : 0);
      for (size_t t = 0; t < q.terms.size() && t < WSR_MAX_TERMS; ++t) {
        int32_t df;
        check(wsr_lookup(h_, q.terms[t].c_str(), &w.list_ids[t], &df));
      }
      docs.insert(docs.end(), doc_ids[i].begin(), doc_ids[i].end());
      off[i + 1] = static_cast<int64_t>(docs.size());
    }
    std::vector<wsr_doc_score> flat(docs.size());
    check(wsr_score_docs(h_, in.data(), static_cast<int32_t>(qs.size()), off.data(), docs.data(), flat.data()));
    std::vector<std::vector<DocScore>> out(qs.size());
    for (size_t i = 0; i < qs.size(); ++i)
      for (int64_t j = off[i]; j < off[i + 1]; ++j) out[i].push_back(DocScore{flat[j].score, flat[j].mask});
    return out;
  }
  std::vector<DocScore> ScoreDocs(const SearchQuery& q, const std::vector<int>& doc_ids) {
    return ScoreDocsBatch({q}, {doc_ids})[0];
  }

  // wsr_search_bool: MUST / SHOULD / MUST_NOT terms with min_should.  Entries
  // and doc_freqs as for a match_any query: a term missing from the index has
  // doc_freq 0 (a missing MUST term: no entries); no terms or n_results <= 0:
  // nothing, doc_freqs unset.  The engine checks the limits.
  std::vector<SearchResult> SearchBool(const std::vector<BoolQuery>& qs) { return SearchBool(qs, {}); }
  // ... restricted to doc sets (wsr_search_bool_filtered): filters[i] is query
  // i's set, nullptr for none; no filters at all is the call above.
  std::vector<SearchResult> SearchBool(const std::vector<BoolQuery>& qs, const std::vector<const DocSet*>& filters) {
    std::vector<wsr_bool_query> in(qs.size());
    std::vector<std::vector<int>> freqs(qs.size());
    int stride = 1;
    for (size_t i = 0; i < qs.size(); ++i) {
      const BoolQuery& q = qs[i];
      wsr_bool_query& w = in[i];
      w = Resolve(q, &freqs[i]);
      w.k = q.n_results < 0 ? 0 : q.n_results;
      if (w.k > stride) stride = w.k;
    }
    std::vector<wsr_hit> hits(qs.size() * stride);
    std::vector<int32_t> nh(qs.size());
    if (filters.empty()) {
      check(wsr_search_bool(h_, in.data(), static_cast<int32_t>(qs.size()), stride, hits.data(), nh.data()));
    } else {
      const std::vector<const wsr_docset*> f = RawFilters(filters, qs.size());
      check(wsr_search_bool_filtered(h_, in.data(), static_cast<int32_t>(qs.size()), f.data(), stride, hits.data(),
                                     nh.data(), 0, nullptr));
    }
    std::vector<SearchResult> out(qs.size());
    for (size_t i = 0; i < qs.size(); ++i) {
      if (qs[i].terms.empty() || in[i].k == 0) continue;
      out[i].doc_freqs = freqs[i];
      for (int j = 0; j < nh[i]; ++j) {
        SearchResultEntry e;
        e.doc_id = hits[i * stride + j].doc_id;
        e.doc_score = hits[i * stride + j].score;
        out[i].entries.push_back(e);
      }
    }
    return out;
  }

  // wsr_count_bool: how many docs match each query under SearchBool's match
  // rule.  n_results is ignored; a term missing from the index is list id -1.
  // On a doc-range shard engine: the matches in the shard's doc range.
  std::vector<int64_t> CountBool(const std::vector<BoolQuery>& qs) { return CountBool(qs, {}); }
  // ... restricted to doc sets (wsr_count_bool_filtered), as SearchBool's filters
  std::vector<int64_t> CountBool(const std::vector<BoolQuery>& qs, const std::vector<const DocSet*>& filters) {
    std::vector<wsr_bool_query> in(qs.size());
    for (size_t i = 0; i < qs.size(); ++i) in[i] = Resolve(qs[i], nullptr);
    std::vector<int64_t> counts(qs.size());
    if (filters.empty()) {
      check(wsr_count_bool(h_, in.data(), static_cast<int32_t>(qs.size()), counts.data()));
    } else {
      const std::vector<const wsr_docset*> f = RawFilters(filters, qs.size());
      check(wsr_count_bool_filtered(h_, in.data(), static_cast<int32_t>(qs.size()), f.data(), counts.data(), 0,
                                    nullptr));
    }
    return counts;
  }

  // wsr_docset_from_ids: the set of the given doc ids of the whole index (any
  // order, duplicates allowed; an id outside the index is refused).
  DocSet MakeDocSet(const std::vector<int32_t>& ids) {
    wsr_docset* s = nullptr;
    check(wsr_docset_from_ids(h_, ids.data(), static_cast<int64_t>(ids.size()), &s));
    return DocSet(h_, s);
  }
  // wsr_docset_from_bool: the docs that match q under SearchBool's match rule
  // (n_results is ignored), intersected with `within` when given.
  DocSet MakeDocSet(const BoolQuery& q, const DocSet* within = nullptr) {
    const wsr_bool_query w = Resolve(q, nullptr);
    wsr_docset* s = nullptr;
    check(wsr_docset_from_bool(h_, &w, within ? within->get() : nullptr, 0, &s));
    return DocSet(h_, s);
  }

  std::vector<SearchResult> SearchBatch(const std::vector<SearchQuery>& qs) {
    std::vector<wsr_query> in(qs.size());
    std::vector<std::vector<int32_t>> more(qs.size());   // terms past WSR_MAX_TERMS
    std::vector<std::vector<int>> freqs(qs.size());
    std::vector<bool> empty(qs.size(), false);
    int stride = 1;
    for (size_t i = 0; i < qs.size(); ++i) {
      const SearchQuery& q = qs[i];
      if (q.terms.size() > WSR_MAX_QUERY_TERMS || q.n_results > WSR_MAX_K)
        throw std::runtime_error("query over the engine limits");
      if (q.match_any && (q.is_phrase || q.return_snippets))
        throw std::runtime_error("wiser_hip: match_any goes with neither is_phrase nor return_snippets");
      if (q.match_any && q.terms.size() > WSR_MAX_OR_TERMS)
        throw std::runtime_error("wiser_hip: more than WSR_MAX_OR_TERMS terms in a match_any query");
      wsr_query& w = in[i];
      w.more_ids = nullptr;
      w.k = q.n_results < 0 ? 0 : q.n_results;
      w.flags = q.match_any ? WSR_QUERY_OR : (q.is_phrase && q.terms.size() > 1) ? WSR_QUERY_PHRASE : 0;
      bool missing = q.terms.empty();
      for (size_t t = 0; t < q.terms.size(); ++t) {
        int32_t id, df;
        check(wsr_lookup(h_, q.terms[t].c_str(), &id, &df));
        if (t < WSR_MAX_TERMS) w.list_ids[t] = id;
        else more[i].push_back(id);
        if (id < 0 && !q.match_any) missing = true;
        freqs[i].push_back(df);
      }
      if (!more[i].empty()) w.more_ids = more[i].data();
      empty[i] = missing || w.k == 0;
      w.n_terms = empty[i] ? 0 : static_cast<int32_t>(q.terms.size());
      if (w.k > stride) stride = w.k;
    }
    std::vector<wsr_hit> hits(qs.size() * stride);
    std::vector<int32_t> nh(qs.size());
    if (!qs.empty())
      check(wsr_search_batch(h_, in.data(), static_cast<int32_t>(qs.size()), stride, hits.data(),
                             nh.data()));
    std::vector<SearchResult> out(qs.size());
    for (size_t i = 0; i < qs.size(); ++i) {
      if (empty[i]) continue;  // vacuum_engine.h:206-215: nothing, doc_freqs unset
      out[i].doc_freqs = freqs[i];
      for (int j = 0; j < nh[i]; ++j) {
        SearchResultEntry e;
        e.doc_id = hits[i * stride + j].doc_id;
        e.doc_score = hits[i * stride + j].score;
        out[i].entries.push_back(e);
      }
    }
    // vacuum_engine.h:248-252: snippets of every entry, the batch at once on the
    // host's threads, one call per distinct n_snippet_passages
    std::map<int, std::vector<int32_t>> groups;   // n_passages -> n_hits masked to that group
    for (size_t i = 0; i < qs.size(); ++i) {
      if (!qs[i].return_snippets || empty[i] || nh[i] == 0) continue;
      auto& g = groups[qs[i].n_snippet_passages];
      if (g.empty()) g.assign(qs.size(), 0);
      g[i] = nh[i];
    }
    for (auto& kv : groups) {
      std::vector<uint64_t> ends(qs.size() * stride);
      uint64_t total = 0;
      std::string buf(1 << 16, '\0');
      int rc = wsr_snippets_batch(h_, in.data(), static_cast<int32_t>(qs.size()), hits.data(), kv.second.data(),
                                  stride, kv.first, 0, &buf[0], buf.size(), ends.data(), &total);
      if (rc == WSR_E_LIMIT && total > buf.size()) {
        buf.assign(total, '\0');
        rc = wsr_snippets_batch(h_, in.data(), static_cast<int32_t>(qs.size()), hits.data(), kv.second.data(),
                                stride, kv.first, 0, &buf[0], buf.size(), ends.data(), &total);
      }
      check(rc);
      uint64_t at = 0;
      for (size_t i = 0; i < qs.size(); ++i)
        for (int j = 0; j < stride; ++j) {
          const uint64_t e = ends[i * stride + j];
          if (j < kv.second[i]) out[i].entries[j].snippet.assign(buf, at, e - at);
          at = e;
        }
    }
    return out;
  }

 private:
  // q by list ids (k left 0); freqs, when given, receives the terms' doc_freqs
  wsr_bool_query Resolve(const BoolQuery& q, std::vector<int>* freqs) const {
    if (q.terms.size() > WSR_MAX_OR_TERMS)
      throw std::runtime_error("wiser_hip: more than WSR_MAX_OR_TERMS terms in a boolean query");
    wsr_bool_query w{};
    w.n_terms = static_cast<int32_t>(q.terms.size());
    w.min_should = q.min_should;
    for (size_t t = 0; t < q.terms.size(); ++t) {
      int32_t df;
      check(wsr_lookup(h_, q.terms[t].first.c_str(), &w.list_ids[t], &df));
      w.role[t] = static_cast<uint8_t>(q.terms[t].second);
      if (freqs) freqs->push_back(df);
    }
    return w;
  }
  static std::vector<const wsr_docset*> RawFilters(const std::vector<const DocSet*>& filters, size_t nq) {
    if (filters.size() != nq) throw std::runtime_error("wiser_hip: one filter (or nullptr) per query");
    std::vector<const wsr_docset*> f(nq, nullptr);
    for (size_t i = 0; i < nq; ++i)
      if (filters[i]) f[i] = filters[i]->get();
    return f;
  }

  std::string dir_;
  int device_;
  int bloom_factor_ = 1;
  wsr_handle* h_ = nullptr;
};

}  // namespace wiser_hip

#endif
