// wsr_score_docs (include/wiser_hip.h): what the engine's BM25 gives each of
// the caller's (query, doc) pairs.  The host plans the call (score_plan.cc:
// checks, the candidates sorted per query and cut into items); one launch of
// score_docs_kernel answers it.
#include <cstring>

#include "engine_impl.h"
#include "score_plan.h"

using namespace wiser;

static_assert(sizeof(wsr_doc_score) == sizeof(DocScore), "wsr_doc_score layout");

extern "C" int wsr_score_docs(wsr_handle* h, const wsr_query* q, int32_t nq, const int64_t* doc_off,
                              const int32_t* docs, wsr_doc_score* out) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  // (no handle lock: the image is read-only after wsr_open and each call works in a context of its own)
  ScorePlan p;
  std::string why;
  const int prc = plan_score_docs(h->view(), h->idx.n_docs(), q, nq, doc_off, docs, &p, &why);
  if (prc) return fail(prc, why);
  const size_t total = p.docs.size();
  if (!total) return WSR_OK;
  if (!out) return fail(WSR_E_INVALID, "null argument");
  if (p.items.empty()) {   // no term of any query has postings here, or no candidate is in the image's range
    std::memset(out, 0, sizeof(wsr_doc_score) * total);
    return WSR_OK;
  }
  std::unique_ptr<ScoreCtx> c = h->score_pool.take();
  try {
    HIP_OK(hipSetDevice(h->device));
    if (!c) {
      c.reset(new ScoreCtx());
      c->st = gpu::make_stream();
    }
    const size_t n_q = p.qs.size(), n_items = p.items.size();
    c->d_qs.reserve(n_q, n_q + n_q / 4);
    c->d_items.reserve(n_items, n_items + n_items / 4);
    if (total > c->d_docs.size()) gpu::alloc_group(total + total / 4, c->d_docs, c->d_index, c->d_out);
    const hipStream_t st = c->st;
    HIP_OK(hipMemcpyAsync(c->d_qs, p.qs.data(), sizeof(ScoreQuery) * n_q, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_items, p.items.data(), sizeof(ScoreItem) * n_items, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_docs, p.docs.data(), sizeof(uint32_t) * total, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(c->d_index, p.index.data(), sizeof(uint32_t) * total, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(c->d_out, 0, sizeof(DocScore) * total, st));   // the rows no item covers: {0.0, 0}
    HIP_OK(launch_score_docs(h->args, c->d_qs, c->d_items, static_cast<uint32_t>(n_items), c->d_docs, c->d_index,
                             c->d_out, st));
    HIP_OK(hipMemcpyAsync(out, c->d_out, sizeof(DocScore) * total, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (const std::exception& e) {
    // (the context goes with what it holds, once its stream is idle)
    if (c && c->st) (void)hipStreamSynchronize(c->st);
    return fail(WSR_E_HIP, e.what());
  }
  h->score_pool.give(std::move(c));
  return WSR_OK;
}
