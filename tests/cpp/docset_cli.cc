// C++ host above the C ABI, for the doc-set mirror of
// include/wiser_hip_engine.hpp (DocSet, MakeDocSet, the filtered SearchBool
// and CountBool): load an index and answer the filtered boolean queries of a
// file.  One query per line: the filter, min_should, then bool_cli's terms
// ("+term" MUST, "-term" MUST_NOT, any other SHOULD).  The filter is "*" (no
// filter), "i:3,1,2" (the set of those doc ids; "i:" is the empty set) or
// "b:+a,-b" (the match set of those terms, min_should 0).  One line per query:
//   <filtered count> | <ids of the query's match set within the filter> | <doc>:<score> ...
// the last part the filtered SearchBool at k = 10, all queries in one call.
// Used by tests/test_gpu_docset.py.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

#include "wiser_hip_engine.hpp"

namespace {
void add_term(wiser_hip::BoolQuery* q, const std::string& t) {
  if (t[0] == '+') q->terms.emplace_back(t.substr(1), wiser_hip::Role::kMust);
  else if (t[0] == '-') q->terms.emplace_back(t.substr(1), wiser_hip::Role::kMustNot);
  else q->terms.emplace_back(t, wiser_hip::Role::kShould);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: docset_cli <index dir> <query file>\n";
    return 2;
  }
  try {
    wiser_hip::VacuumHipEngine eng(argv[1]);
    eng.Load();
    std::vector<wiser_hip::BoolQuery> qs;
    std::vector<std::unique_ptr<wiser_hip::DocSet>> sets;
    std::vector<const wiser_hip::DocSet*> filters;
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) {
      std::istringstream ss(line);
      std::string f;
      wiser_hip::BoolQuery q;
      ss >> f >> q.min_should;
      for (std::string t; ss >> t;) add_term(&q, t);
      qs.push_back(q);
      std::unique_ptr<wiser_hip::DocSet> s;
      if (f.rfind("i:", 0) == 0) {
        std::vector<int32_t> ids;
        std::istringstream is(f.substr(2));
        for (std::string x; std::getline(is, x, ',');) ids.push_back(std::stoi(x));
        s.reset(new wiser_hip::DocSet(eng.MakeDocSet(ids)));
      } else if (f.rfind("b:", 0) == 0) {
        wiser_hip::BoolQuery fq;
        std::istringstream is(f.substr(2));
        for (std::string x; std::getline(is, x, ',');) add_term(&fq, x);
        s.reset(new wiser_hip::DocSet(eng.MakeDocSet(fq)));
      }
      filters.push_back(s.get());
      sets.push_back(std::move(s));
    }
    const std::vector<int64_t> counts = eng.CountBool(qs, filters);
    const std::vector<wiser_hip::SearchResult> res = eng.SearchBool(qs, filters);
    for (size_t i = 0; i < qs.size(); ++i) {
      std::printf("%lld |", static_cast<long long>(counts[i]));
      const wiser_hip::DocSet m = eng.MakeDocSet(qs[i], filters[i]);
      for (const int32_t d : m.Ids()) std::printf(" %d", d);
      std::printf(" |");
      for (const auto& e : res[i].entries) std::printf(" %d:%.17g", e.doc_id, e.doc_score);
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::cerr << e.what() << "\n";
    return 1;
  }
  return 0;
}
