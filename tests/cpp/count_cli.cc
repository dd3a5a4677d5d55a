// C++ host above the C ABI, for VacuumHipEngine::CountBool
// (include/wiser_hip_engine.hpp): load an index and count the matches of the
// boolean queries of a file in one CountBool call.  The query file is
// bool_cli's: one query per line, min_should, then the terms separated by
// spaces, "+term" a MUST term, "-term" a MUST_NOT term, any other a SHOULD
// term.  One line per query: its count.  Used by tests/test_gpu_count.py.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "wiser_hip_engine.hpp"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: count_cli <index dir> <query file>\n";
    return 2;
  }
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
      qs.push_back(q);
    }
    for (const int64_t c : eng.CountBool(qs)) std::printf("%lld\n", static_cast<long long>(c));
  } catch (const std::exception& e) {
    std::cerr << e.what() << "\n";
    return 1;
  }
  return 0;
}
