// C++ host above the C ABI, for VacuumHipEngine::ScoreDocsBatch
// (include/wiser_hip_engine.hpp): load an index, run the queries of a log file
// (one query per line, terms separated by spaces) as SearchBatch, then ask
// ScoreDocsBatch about each query's own result docs.  Per query two lines:
// "doc:score(hex)" per hit, then "doc:score(hex):mask" per scored doc.
// Used by tests/test_gpu_score_docs.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "wiser_hip_engine.hpp"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: score_cli <index dir> <query log> [k]\n";
    return 2;
  }
  const int k = argc > 3 ? std::atoi(argv[3]) : 10;
  try {
    wiser_hip::VacuumHipEngine eng(argv[1]);
    eng.Load();
    std::vector<wiser_hip::SearchQuery> qs;
    std::ifstream in(argv[2]);
    for (std::string line; std::getline(in, line);) {
      std::istringstream ss(line);
      wiser_hip::SearchQuery q;
      for (std::string t; ss >> t;) q.terms.push_back(t);
      q.n_results = k;
      qs.push_back(q);
    }
    const auto res = eng.SearchBatch(qs);
    std::vector<std::vector<int>> ids(res.size());
    for (size_t q = 0; q < res.size(); ++q)
      for (size_t i = 0; i < res[q].Size(); ++i) ids[q].push_back(res[q][i].doc_id);
    const auto scored = eng.ScoreDocsBatch(qs, ids);
    for (size_t q = 0; q < res.size(); ++q) {
      for (size_t i = 0; i < res[q].Size(); ++i)
        std::printf("%s%d:%a", i ? " " : "", res[q][i].doc_id, res[q][i].doc_score);
      std::printf("\n");
      for (size_t i = 0; i < scored[q].size(); ++i)
        std::printf("%s%d:%a:%u", i ? " " : "", ids[q][i], scored[q][i].score, scored[q][i].mask);
      std::printf("\n");
    }
    // the single-query form gives the batch's answer
    if (!qs.empty()) {
      const auto one = eng.ScoreDocs(qs[0], ids[0]);
      if (one.size() != scored[0].size()) throw std::runtime_error("ScoreDocs: size differs");
      for (size_t i = 0; i < one.size(); ++i)
        if (one[i].score != scored[0][i].score || one[i].mask != scored[0][i].mask)
          throw std::runtime_error("ScoreDocs differs from ScoreDocsBatch");
    }
  } catch (const std::exception& e) {
    std::cerr << e.what() << "\n";
    return 1;
  }
  return 0;
}
