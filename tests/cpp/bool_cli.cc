// C++ host above the C ABI, for VacuumHipEngine::SearchBool
// (include/wiser_hip_engine.hpp): load an index and run the boolean queries of
// a file as one SearchBool call.  One query per line: min_should, then the
// terms separated by spaces, "+term" a MUST term, "-term" a MUST_NOT term,
// any other a SHOULD term.  Per query two lines: "doc:score(hex)" per hit,
// then the doc_freqs.  Used by tests/test_gpu_bool.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "wiser_hip_engine.hpp"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: bool_cli <index dir> <query file> [k]\n";
    return 2;
  }
  const int k = argc > 3 ? std::atoi(argv[3]) : 10;
  try {
    wiser_hip::VacuumHipEngine eng(argv[1]);
    eng.Load();
    std::vector<wiser_hip::BoolQuery> qs;
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) {
      std::istringstream ss(line);
      wiser_hip::BoolQuery q;
      ss >> q.min_should;
      for (std::string t; ss >> t;) {
        if (t[0] == '+') q.terms.emplace_back(t.substr(1), wiser_hip::Role::kMust);
        else if (t[0] == '-') q.terms.emplace_back(t.substr(1), wiser_hip::Role::kMustNot);
        else q.terms.emplace_back(t, wiser_hip::Role::kShould);
      }
      q.n_results = k;
      qs.push_back(q);
    }
    const auto res = eng.SearchBool(qs);
    for (size_t q = 0; q < res.size(); ++q) {
      for (size_t i = 0; i < res[q].Size(); ++i)
        std::printf("%s%d:%a", i ? " " : "", res[q][i].doc_id, res[q][i].doc_score);
      std::printf("\n");
      for (size_t i = 0; i < res[q].doc_freqs.size(); ++i) std::printf("%s%d", i ? " " : "", res[q].doc_freqs[i]);
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::cerr << e.what() << "\n";
    return 1;
  }
  return 0;
}
