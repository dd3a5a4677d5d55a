// C ABI (include/wiser_hip.h) over the HIP engine: index load + HBM upload,
// resident query batches, kernel launches, result download.  (Doc-range shard
// steps and their communicators: shard_exchange.cc.)
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <cstdio>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "engine_impl.h"
#include "format.h"
#include "writer.h"

using namespace wiser;

namespace wiser {
thread_local std::string g_err;
// (server.cc: a request failed on the dispatcher thread; its caller's thread
// gets the message)
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace wiser

namespace {

// fills dst from a host array (an empty one: a one-element placeholder); the bytes allocated
template <class T, class A>
uint64_t dev_upload(gpu::DevBuf<T>& dst, const std::vector<T, A>& src) {
  dst.alloc(std::max<size_t>(src.size(), 1));
  if (!src.empty()) HIP_OK(hipMemcpy(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return dst.bytes();
}

}  // namespace

namespace {
// bytes dev_upload allocates for a host array (at least one element)
template <class V>
uint64_t dev_bytes(const V& v) {
  return std::max<uint64_t>(v.size(), 1) * sizeof(typename V::value_type);
}

// the image's HBM buffers, per kind, as wsr_open allocates them
wsr_image_info image_info_of(const HostImage& img, size_t n_c4) {
  wsr_image_info o{};
  if (img.has_blooms) o.pos_bytes += dev_bytes(img.blm) + dev_bytes(img.blm_hash);
  if (img.has_positions)
    o.pos_bytes += dev_bytes(img.pos_blob) + dev_bytes(img.pos_lists) + dev_bytes(img.pos_pk) +
                   dev_bytes(img.pos_tail) + dev_bytes(img.pos_start);
  o.dense_bytes = dev_bytes(img.dense) + dev_bytes(img.dense_rank) + dev_bytes(img.bkt);
  o.tf8_bytes = dev_bytes(img.tf8);
  o.blob_bytes = dev_bytes(img.blob);
  o.plen_bytes = dev_bytes(img.plen);
  o.dir_bytes = dev_bytes(img.tails) + dev_bytes(img.lists) + dev_bytes(img.blocks) + dev_bytes(img.blk_last) +
                dev_bytes(img.blk_meta) + dev_bytes(img.bmax) + std::max<uint64_t>(n_c4, 1);
  o.impact_bytes = dev_bytes(img.impact);   // (a part of dir_bytes)
  o.dir_bytes += o.impact_bytes;
  if (!img.doc16.empty()) {   // (a part of dir_bytes, as are the lists' runs in it)
    o.doc16_bytes = dev_bytes(img.doc16);
    o.dir_bytes += o.doc16_bytes + dev_bytes(img.d16_blk);
  }
  o.dense_lists = img.dense_lists;
  o.n_lists = static_cast<uint32_t>(img.lists.size());
  o.total_bytes = o.blob_bytes + o.dense_bytes + o.tf8_bytes + o.plen_bytes + o.dir_bytes + o.pos_bytes;
  return o;
}

// the load-time knobs of wsr_open (environment)
uint32_t dense_div_knob() { return static_cast<uint32_t>(env_number("WSR_DENSE_DIV", 8192)); }
uint64_t dense_budget_knob() { return static_cast<uint64_t>(env_number("WSR_DENSE_BUDGET_GB", 48) * 1e9); }
// WSR_DOC16=0: no 16-bit doc ids, every driver's doc ids are unpacked (HostImage::doc16)
bool doc16_knob() { return env_number("WSR_DOC16", 1) != 0; }
}  // namespace

extern "C" {

const char* wsr_last_error(void) { return g_err.c_str(); }
const char* wsr_version(void) { return "wiser-hip 0.2 (gfx950)"; }

int wsr_image_info_get(wsr_handle* h, wsr_image_info* out) {
  if (!h || !out) return fail(WSR_E_INVALID, "null argument");
  *out = h->info;
  out->total_bytes = out->blob_bytes + out->dense_bytes + out->tf8_bytes + out->plen_bytes + out->dir_bytes +
                     out->pos_bytes;
  return WSR_OK;
}


int wsr_image_size(const char* dir, uint32_t doc_lo, uint32_t doc_hi, int32_t positions, int32_t bloom_factor,
                   int32_t threads, wsr_image_info* out) {
  if (!dir || !out) return fail(WSR_E_INVALID, "null argument");
  try {
    VacuumIndex idx;
    idx.open(dir);
    const int t = threads > 0 ? threads : static_cast<int>(std::thread::hardware_concurrency());
    const HostImage img = build_image(idx, doc_lo, doc_hi ? doc_hi : 0xFFFFFFFFu, std::min(t, 32), dense_div_knob(),
                                      positions != 0, dense_budget_knob(), positions && bloom_factor > 0, 0,
                                      doc16_knob());
    *out = image_info_of(img, idx.char4_lengths().size());
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_runtime_info(char* buf, int32_t cap) {
  if (!buf || cap <= 0) return fail(WSR_E_INVALID, "null argument");
  int ver = 0;
  (void)hipRuntimeGetVersion(&ver);
  Dl_info hip{}, rccl{};
  const char* hp = dladdr(reinterpret_cast<void*>(&hipRuntimeGetVersion), &hip) && hip.dli_fname ? hip.dli_fname : "?";
  const char* rp = dladdr(reinterpret_cast<void*>(&ncclGetUniqueId), &rccl) && rccl.dli_fname ? rccl.dli_fname : "?";
  std::snprintf(buf, static_cast<size_t>(cap), "hipRuntimeGetVersion=%d libamdhip64=%s librccl=%s", ver, hp, rp);
  return WSR_OK;
}

int wsr_open(const char* dir, const wsr_open_opts* opts, wsr_handle** out) {
  if (!dir || !out) return fail(WSR_E_INVALID, "null argument");
  *out = nullptr;
  std::unique_ptr<wsr_handle> h(new wsr_handle());
  try {
    h->idx.open(dir);
    h->docs.open(dir);
    h->rows.reset(new SkipRowCache(h->idx));
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  try {
    const int dev = opts ? opts->device : 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= dev)
      return fail(WSR_E_HIP, "no HIP device " + std::to_string(dev) + " (MI355X required; no CPU fallback)");
    HIP_OK(hipSetDevice(dev));
    h->device = dev;
    uint32_t lo = opts ? opts->doc_lo : 0, hi = opts ? opts->doc_hi : 0;
    if (hi == 0) hi = 0xFFFFFFFFu;
    int threads = opts && opts->threads > 0 ? opts->threads : static_cast<int>(std::thread::hardware_concurrency());
    // probe structures (bitmaps, offset buckets): lists with >= span/div
    // postings (WSR_DENSE_DIV, 0 = off), probed when >= ratio x the driver's
    // blocks (WSR_DENSE_RATIO).  8192 since round 4's buckets made a sparse
    // list's structure cheap (~6 B per posting + 8 B per 256 docs): on the C3
    // stand-in C5 6.1 -> 10.1 M q/s against 2048 (its phrases' lists become
    // lean), headline and C4 within 1 %, image 10.1 -> 14.0 GB (16384 and
    // 32768: C5 the same, headline +0.4 %, 17.6 / 23.0 GB;
    // profiles/r04k/, r04l/).  WSR_DENSE_BUDGET_GB caps their HBM, longest
    // lists first (48 GB)
    const uint32_t dense_div = dense_div_knob();
    const uint64_t dense_budget = dense_budget_knob();
    const float dense_ratio = static_cast<float>(env_number("WSR_DENSE_RATIO", 1.0));
    h->positions = opts && opts->positions;
    const uint32_t bloom_factor = opts && opts->bloom_factor > 0 ? static_cast<uint32_t>(opts->bloom_factor) : 0u;
    // (the bitmaps are sized to what the device has free: an image larger than
    // the free HBM drops the bitmaps of its shortest dense lists first)
    size_t hbm_free = 0, hbm_total = 0;
    HIP_OK(hipMemGetInfo(&hbm_free, &hbm_total));
    HostImage img = build_image(h->idx, lo, hi, std::min(threads, 32), dense_div, h->positions, dense_budget,
                                bloom_factor > 0, hbm_free, doc16_knob());
    if (img.has_blooms) {   // (counted with the position boxes)
      h->info.pos_bytes += dev_upload(h->d_blm, img.blm);
      h->info.pos_bytes += dev_upload(h->d_blm_hash, img.blm_hash);
      h->args.blm = reinterpret_cast<const uint4*>(h->d_blm.get());
      h->args.blm_hash = reinterpret_cast<const uint2*>(h->d_blm_hash.get());
      h->args.blm_bits = img.blm_bits;
      h->args.blm_hashes = img.blm_hashes;
      h->args.bloom_factor = bloom_factor;
      big_vector<uint8_t>().swap(img.blm);
    }
    if (h->positions) {
      h->info.pos_bytes += dev_upload(h->d_pos_blob, img.pos_blob);
      h->info.pos_bytes += dev_upload(h->d_pos_lists, img.pos_lists);
      h->info.pos_bytes += dev_upload(h->d_pos_pk, img.pos_pk);
      h->info.pos_bytes += dev_upload(h->d_pos_tail, img.pos_tail);
      h->info.pos_bytes += dev_upload(h->d_pos_start, img.pos_start);
      h->args.pos_blob = h->d_pos_blob.get();
      h->args.pos_lists = h->d_pos_lists.get();
      h->args.pos_pk = reinterpret_cast<const uint2*>(h->d_pos_pk.get());
      h->args.pos_tail = h->d_pos_tail.get();
      h->args.pos_start = reinterpret_cast<const uint2*>(h->d_pos_start.get());
      h->pos_bytes = img.pos_list_bytes;
      std::vector<uint8_t>().swap(img.pos_blob);
      std::vector<uint32_t>().swap(img.pos_start);
    }
    h->info.dense_bytes = dev_upload(h->d_dense, img.dense);
    h->info.dense_bytes += dev_upload(h->d_dense_rk, img.dense_rank);
    h->info.dense_bytes += dev_upload(h->d_bkt, img.bkt);
    h->info.tf8_bytes = dev_upload(h->d_tf8, img.tf8);
    h->dense_lists = img.dense_lists;
    h->info.dense_lists = img.dense_lists;
    h->info.n_lists = static_cast<uint32_t>(img.lists.size());
    h->args.dense = h->d_dense.get();
    h->args.dense_rk = h->d_dense_rk.get();
    h->args.bkt = reinterpret_cast<const uint2*>(h->d_bkt.get());
    h->args.tf8 = h->d_tf8.get();
    h->args.dense_span = img.dense_span;
    h->args.dense_ratio = dense_ratio;
    h->args.seg_cap = kSegCost;
    h->info.blob_bytes = dev_upload(h->d_blob, img.blob);
    h->info.plen_bytes = dev_upload(h->d_plen, img.plen);
    h->args.plen = h->d_plen.get();
    h->info.impact_bytes = dev_upload(h->d_impact, img.impact);
    h->info.dir_bytes += h->info.impact_bytes;
    h->args.impact = h->d_impact.get();
    if (!img.doc16.empty()) {   // (WSR_DOC16=0, or no eligible list: both stay null, every list ineligible)
      h->info.doc16_bytes = dev_upload(h->d_doc16, img.doc16);
      h->info.dir_bytes += h->info.doc16_bytes + dev_upload(h->d_d16_blk, img.d16_blk);
      h->args.doc16 = h->d_doc16.get();
      h->args.d16_blk = h->d_d16_blk.get();
      big_vector<uint16_t>().swap(img.doc16);
    }
    {   // (rounded down: the other terms' bound falls as the norm grows)
      float nm = static_cast<float>(img.norm_min);
      if (static_cast<double>(nm) > img.norm_min) nm = std::nextafter(nm, 0.0f);
      h->args.norm_min = nm;
    }
    h->info.dir_bytes += dev_upload(h->d_bmax, img.bmax);
    h->args.bmax = h->d_bmax.get();
    h->info.dir_bytes += dev_upload(h->d_tails, img.tails);
    h->args.tails = h->d_tails.get();
    h->info.dir_bytes += dev_upload(h->d_lists, img.lists);
    h->info.dir_bytes += dev_upload(h->d_blocks, img.blocks);
    h->info.dir_bytes += dev_upload(h->d_last, img.blk_last);
    h->info.dir_bytes += dev_upload(h->d_meta, img.blk_meta);
    h->info.dir_bytes += dev_upload(h->d_c4, h->idx.char4_lengths());
    std::vector<double> cache(h->idx.bm25_cache(), h->idx.bm25_cache() + 256);
    dev_upload(h->d_cache, cache);
    h->lists = img.lists;
    h->blocks.assign(img.blocks.begin(), img.blocks.end());
    h->meta.assign(img.blk_meta.begin(), img.blk_meta.end());
    h->list_bytes = img.list_bytes;
    h->args.blob = h->d_blob.get();
    h->args.lists = h->d_lists.get();
    h->args.blocks = h->d_blocks.get();
    h->args.blk_last = h->d_last.get();
    h->args.blk_meta = h->d_meta.get();
    h->args.c4 = h->d_c4.get();
    h->args.cache = h->d_cache.get();
    h->args.n_c4 = static_cast<uint32_t>(h->idx.char4_lengths().size());
    h->args.n_lists = static_cast<uint32_t>(img.lists.size());
    h->args.doc_lo = lo;
    h->args.doc_hi = hi;
    h->args.avg = h->idx.avg_length();
    h->stream = gpu::make_stream();

    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, dev));
    int occ = segment_kernel_occupancy();
    if (occ < 1) occ = 1;
    h->grid = prop.multiProcessorCount * std::min(occ, 32);
    // general workers hold 12 KB of LDS each: at most 4 per CU, so that the
    // concurrent lean kernel keeps its occupancy
    // (one workgroup per CU past that: it starts as the first resident ones
    // leave; C4 +1.6 %, the mixed log +0.6 %, the rest unchanged,
    // profiles/r05/leg_ab.txt r05ar / r05as)
    const int gen_per_cu = static_cast<int>(env_number("WSR_GEN_PER_CU", 4));
    h->gen_cap = prop.multiProcessorCount * std::max(1, std::min(std::min(occ, 32), gen_per_cu) + 1);
    int locc = lean_kernel_occupancy(false);
    if (locc < 1) locc = 1;
    h->lean_wgs = prop.multiProcessorCount * std::min(locc, 16);
    // the phrase instance holds more registers: its resident grid is smaller
    // (workgroups past it would start only as resident ones leave)
    int pocc = lean_kernel_occupancy(true);
    if (pocc < 1) pocc = 1;
    h->lean_wgs_ph = prop.multiProcessorCount * std::min(std::min(pocc, locc), 16);
    // Batches whose conjunctive items are all two-term (the headline's) run one
    // workgroup per CU past the resident grid: it starts as the first resident
    // waves leave and takes items from the queue's tail (C3 24.0 -> 24.5 M q/s,
    // C2 and C4 unchanged; 2 to 11 more: no better, 11 -6 %; single-term
    // batches -2 %, so they keep the resident grid: profiles/r05/leg_ab.txt r05u-w)
    h->lean_wgs_two = prop.multiProcessorCount * std::min(locc + 1, 16);
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());   // (h goes with what it got)
  }
  *out = h.release();
  return WSR_OK;
}

void wsr_close(wsr_handle* h) {
  if (!h) return;
  for (wsr_batch* b : h->pool) wsr_batch_destroy(h, b);
  h->pool.clear();
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

int wsr_term_count(wsr_handle* h, int32_t* out) {
  if (!h || !out) return fail(WSR_E_INVALID, "null argument");
  *out = h->idx.n_lists();
  return WSR_OK;
}

int wsr_n_docs(wsr_handle* h, int32_t* out) {
  if (!h || !out) return fail(WSR_E_INVALID, "null argument");
  *out = h->idx.n_docs();
  return WSR_OK;
}

int wsr_lookup(wsr_handle* h, const char* term, int32_t* list_id, int32_t* df) {
  if (!h || !term) return fail(WSR_E_INVALID, "null argument");
  const int32_t id = h->idx.find(term);
  if (list_id) *list_id = id;
  if (df) *df = id < 0 ? 0 : static_cast<int32_t>(h->idx.df(id));
  return WSR_OK;
}

// ------------------------------------------------------------ snippets ----
// Host stage after the top-k, as in the reference (vacuum_engine.h:243-253).
struct wsr_docs {
  VacuumIndex idx;
  DocStore docs;
  std::unique_ptr<SkipRowCache> rows;
};

namespace {
int copy_out(const std::string& s, char* out, int32_t cap, int32_t* len) {
  if (len) *len = static_cast<int32_t>(s.size());
  if (out && cap > 0) std::memcpy(out, s.data(), std::min<size_t>(s.size(), static_cast<size_t>(cap)));
  return WSR_OK;
}

int check_snippet_query(const VacuumIndex& idx, const DocStore& docs, const wsr_query* q) {
  if (q->n_terms < 1 || q->n_terms > WSR_MAX_QUERY_TERMS) return fail(WSR_E_LIMIT, "bad term count");
  if (q->n_terms > WSR_MAX_TERMS && !q->more_ids) return fail(WSR_E_INVALID, "more_ids missing");
  // (the highlighter takes a bag of every term in the doc)
  if (q->flags & WSR_QUERY_OR) return fail(WSR_E_INVALID, "no snippets for a disjunctive query");
  if (!docs.is_open()) return fail(WSR_E_INVALID, "the index has no doc store (my.fdx / my.fdt)");
  for (int32_t id : query_terms(*q))
    if (id < 0 || id >= idx.n_lists())
      return fail(WSR_E_INVALID, "a query term is not in the index (no result entries)");
  return WSR_OK;
}

int snippet_of(const VacuumIndex& idx, const SkipRowCache& rows, const DocStore& docs, const wsr_query* q,
               int32_t doc, int32_t n_passages, char* out, int32_t cap, int32_t* len) {
  if (!q || !len || n_passages < 0) return fail(WSR_E_INVALID, "bad snippet arguments");
  const int rc = check_snippet_query(idx, docs, q);
  if (rc != WSR_OK) return rc;
  try {
    const std::vector<int32_t> ids = query_terms(*q);
    return copy_out(make_snippet(idx, rows, docs, ids.data(), q->n_terms,
                                 (q->flags & WSR_QUERY_PHRASE) != 0, doc, n_passages),
                    out, cap, len);
  } catch (const std::exception& e) {
    return fail(WSR_E_INVALID, e.what());
  }
}

int doc_text(const DocStore& docs, int32_t doc, char* out, int32_t cap, int32_t* len) {
  if (!len) return fail(WSR_E_INVALID, "null argument");
  try {
    return copy_out(docs.get(doc), out, cap, len);
  } catch (const std::exception& e) {
    return fail(WSR_E_INVALID, e.what());
  }
}
}  // namespace

int wsr_snippet(wsr_handle* h, const wsr_query* q, int32_t doc, int32_t n_passages, char* out,
                int32_t cap, int32_t* len) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  return snippet_of(h->idx, *h->rows, h->docs, q, doc, n_passages, out, cap, len);
}

int wsr_snippets_batch(wsr_handle* h, const wsr_query* q, int32_t nq, const wsr_hit* hits,
                       const int32_t* n_hits, int32_t stride, int32_t n_passages, int32_t threads,
                       char* buf, uint64_t cap, uint64_t* ends, uint64_t* total) {
  if (!h || (nq > 0 && (!q || !hits || !n_hits || !ends)) || !total || nq < 0 || stride <= 0 ||
      n_passages < 0)
    return fail(WSR_E_INVALID, "bad snippet batch arguments");
  std::vector<std::pair<int32_t, int32_t>> work;   // (query, entry)
  for (int32_t i = 0; i < nq; ++i) {
    if (n_hits[i] < 0 || n_hits[i] > stride) return fail(WSR_E_INVALID, "bad hit count");
    if (n_hits[i] == 0) continue;
    const int rc = check_snippet_query(h->idx, h->docs, &q[i]);
    if (rc != WSR_OK) return rc;
    for (int32_t j = 0; j < n_hits[i]; ++j) work.emplace_back(i, j);
  }
  std::vector<std::string> out(static_cast<size_t>(nq) * stride);
  std::atomic<size_t> next{0};
  std::mutex err_mu;
  std::string err;
  auto run = [&]() {
    for (size_t w; (w = next.fetch_add(1)) < work.size();) {
      const int32_t i = work[w].first, j = work[w].second;
      try {
        const std::vector<int32_t> ids = query_terms(q[i]);
        out[static_cast<size_t>(i) * stride + j] =
            make_snippet(h->idx, *h->rows, h->docs, ids.data(), q[i].n_terms,
                         (q[i].flags & WSR_QUERY_PHRASE) != 0, hits[static_cast<size_t>(i) * stride + j].doc_id,
                         n_passages);
      } catch (const std::exception& e) {
        std::lock_guard<std::mutex> g(err_mu);
        if (err.empty()) err = e.what();
      }
    }
  };
  int nt = threads > 0 ? threads : static_cast<int>(std::thread::hardware_concurrency());
  nt = std::max(1, std::min<int>(nt, std::min<size_t>(64, work.size())));
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(run);
  run();
  for (auto& t : pool) t.join();
  if (!err.empty()) return fail(WSR_E_INVALID, err);
  uint64_t n = 0;
  for (const auto& s : out) n += s.size();
  *total = n;
  if (n > cap) return fail(WSR_E_LIMIT, "snippet buffer too small (see *total)");
  uint64_t at = 0;
  for (size_t e = 0; e < out.size(); ++e) {
    if (!out[e].empty()) std::memcpy(buf + at, out[e].data(), out[e].size());
    at += out[e].size();
    ends[e] = at;
  }
  return WSR_OK;
}

int wsr_doc_get(wsr_handle* h, int32_t doc, char* out, int32_t cap, int32_t* len) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  return doc_text(h->docs, doc, out, cap, len);
}

int wsr_docs_open(const char* dir, wsr_docs** out) {
  if (!dir || !out) return fail(WSR_E_INVALID, "null argument");
  *out = nullptr;
  std::unique_ptr<wsr_docs> d(new wsr_docs());
  try {
    d->idx.open(dir);
    if (!d->docs.open(dir)) return fail(WSR_E_IO, std::string("no doc store in ") + dir);
    d->rows.reset(new SkipRowCache(d->idx));
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  *out = d.release();
  return WSR_OK;
}

void wsr_docs_close(wsr_docs* d) { delete d; }

int wsr_docs_lookup(wsr_docs* d, const char* term, int32_t* list_id, int32_t* df) {
  if (!d || !term) return fail(WSR_E_INVALID, "null argument");
  const int32_t id = d->idx.find(term);
  if (list_id) *list_id = id;
  if (df) *df = id < 0 ? 0 : static_cast<int32_t>(d->idx.df(id));
  return WSR_OK;
}

int wsr_docs_snippet(wsr_docs* d, const wsr_query* q, int32_t doc, int32_t n_passages, char* out,
                     int32_t cap, int32_t* len) {
  if (!d) return fail(WSR_E_INVALID, "null argument");
  return snippet_of(d->idx, *d->rows, d->docs, q, doc, n_passages, out, cap, len);
}

int wsr_docs_get(wsr_docs* d, int32_t doc, char* out, int32_t cap, int32_t* len) {
  if (!d) return fail(WSR_E_INVALID, "null argument");
  return doc_text(d->docs, doc, out, cap, len);
}

int wsr_highlight(const int32_t* pairs, const int32_t* counts, int32_t n_terms, int32_t n_passages,
                  const char* text, char* out, int32_t cap, int32_t* len) {
  if ((!pairs && n_terms > 0) || (!counts && n_terms > 0) || !text || !len || n_terms < 0)
    return fail(WSR_E_INVALID, "null argument");
  try {
    std::vector<std::vector<OffsetPair>> t(n_terms);
    for (int32_t i = 0; i < n_terms; ++i)
      for (int32_t j = 0; j < counts[i]; ++j, pairs += 2) t[i].emplace_back(pairs[0], pairs[1]);
    return copy_out(highlight_offsets(t, n_passages, text), out, cap, len);
  } catch (const std::exception& e) {
    return fail(WSR_E_INVALID, e.what());
  }
}

int wsr_list_bytes(wsr_handle* h, int32_t id, uint64_t* out) {
  if (!h || !out) return fail(WSR_E_INVALID, "null argument");
  *out = (id >= 0 && id < static_cast<int32_t>(h->list_bytes.size())) ? h->list_bytes[id] : 0;
  return WSR_OK;
}

int wsr_impact_byte(double avg, uint32_t tf, uint32_t c4, uint32_t* byte, double* value) {
  if (!byte || !value || c4 > 255 || !(avg > 0.0)) return fail(WSR_E_INVALID, "bad impact arguments");
  *byte = impact_byte(tf, bm25_norm(static_cast<uint8_t>(c4), avg));
  *value = impact_value(*byte);
  return WSR_OK;
}

int wsr_batch_create(wsr_handle* h, int32_t max_q, int32_t stride, wsr_batch** out) {
  if (!h || !out || max_q <= 0 || stride <= 0 || stride > WSR_MAX_K)
    return fail(WSR_E_INVALID, "bad batch arguments");
  std::lock_guard<std::mutex> g(h->mu);
  std::unique_ptr<wsr_batch> b(new wsr_batch());
  try {
    HIP_OK(hipSetDevice(h->device));
    b->max_q = max_q;
    b->stride = stride;
    b->d_qb.alloc(sizeof(QueryIn) * max_q);
    b->d_plan.alloc(max_q);
    b->d_desc.alloc(max_q);
    b->d_part.alloc((max_q + kPlanThreads - 1) / kPlanThreads + 1);
    b->d_ctr.alloc(kNumCounters + kMaxOwners);   // + shard fill counters
    b->h_ctr.alloc(kNumCounters);
    b->d_hits.alloc(static_cast<size_t>(max_q) * stride);
    b->d_nhits.alloc(max_q);
    b->d_qdone.alloc(max_q);
    b->d_tinyq.alloc(2 * static_cast<size_t>(max_q));
    b->d_stats.alloc(static_cast<size_t>(kStatStride) *
                     (std::max(std::max(h->grid, h->gen_cap), 1) +   // (seg_grid <= gen_cap)
                      kLeanWaves * (std::max(h->lean_wgs_two, 1) + std::max(h->lean_wgs_ph, 1))));
    for (auto& e : b->ev) e = gpu::make_event(true);
    b->st = gpu::make_stream();   // (this order: see wsr_batch::st)
    b->st2 = gpu::make_stream();
    b->st_pad = gpu::make_stream();
    for (gpu::Event* e : {&b->fork, &b->join, &b->join_ph}) *e = gpu::make_event();
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());   // (b goes with what it got)
  }
  *out = b.release();
  return WSR_OK;
}

void wsr_batch_destroy(wsr_handle* h, wsr_batch* b) {
  if (!b) return;
  if (b->x.join()) (void)hipEventSynchronize(b->x.ev[1]);   // a shard step's exchange reads its buffers
  if (b->st) (void)hipStreamSynchronize(b->st);
  if (b->st2) (void)hipStreamSynchronize(b->st2);
  if (b->st_pad) (void)hipStreamSynchronize(b->st_pad);
  delete b;
}

int wsr_check_query(wsr_handle* h, const wsr_query* q) {
  if (!h || !q) return fail(WSR_E_INVALID, "null argument");
  std::string why;
  const int rc = check_query(h->view(), *q, &why);
  return rc ? fail(rc, why) : WSR_OK;
}

// plan (batch_plan.cc: everything that depends on the queries alone), join
// the batch's earlier work, grow the buffers and copy, commit the class
int wsr_batch_upload(wsr_handle* h, wsr_batch* b, const wsr_query* q, int32_t nq) {
  if (!h || !b || (nq > 0 && !q) || nq < 0 || nq > b->max_q)
    return fail(WSR_E_INVALID, "bad upload arguments");
  // (no handle lock: the handle's image is read-only after wsr_open and the
  // batch belongs to the caller, so threads with their own batches pipeline)
  UploadPlan p;
  std::string why;
  const int prc = plan_upload(h->view(), q, nq, b->stride, b->seg_cap, &p, &why);
  if (prc) return fail(prc, why);
  try {
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(b->st));
    if (b->x.join()) HIP_OK(hipEventSynchronize(b->x.ev[1]));   // a shard step's exchange + replay
    // (on-demand buffers: a failure leaves the buffer empty, so the next upload allocates again)
    b->d_events.reserve(p.ev_need, p.ev_need + p.ev_need / 4 + 4096);
    if (p.items_need > b->d_evcnt.size() || !b->d_evcnt)
      gpu::alloc_group(p.items_need + p.items_need / 4 + 1024, b->d_evcnt, b->d_itemq, b->d_pub);
    if (p.cls.has_phrase && !b->d_ph)   // one per general workgroup
      b->d_ph.alloc(kPhraseScratch * static_cast<size_t>(std::max(h->gen_cap, 1)));
    // (the term table of long queries follows the QueryIn array)
    b->d_qb.reserve(p.q_bytes, p.q_bytes + p.q_bytes / 4);
    if (!p.orq.empty()) {   // (a batch without a disjunctive query allocates nothing here)
      const size_t n_or = p.orq.size(), n_items = p.or_items.size();
      if (n_items > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "over 2^32 disjunctive work items");
      b->d_orq.reserve(n_or, n_or + n_or / 4);
      if (n_items > b->d_oritem.size()) gpu::alloc_group(n_items + n_items / 4 + 64, b->d_oritem, b->d_orevcnt);
      b->d_orev.reserve(p.or_ev, p.or_ev + p.or_ev / 4);
      if (!b->d_orstat) b->d_orstat.alloc(kNumOrStats);
      HIP_OK(hipMemcpy(b->d_orq, p.orq.data(), sizeof(OrQuery) * n_or, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(b->d_oritem, p.or_items.data(), sizeof(OrItem) * n_items, hipMemcpyHostToDevice));
    }
    if (nq) HIP_OK(hipMemcpy(b->d_q(), p.in.data(), sizeof(QueryIn) * nq, hipMemcpyHostToDevice));
    if (!p.ext.empty())
      HIP_OK(hipMemcpy(reinterpret_cast<char*>(b->d_q()) + sizeof(QueryIn) * nq, p.ext.data(),
                       sizeof(int32_t) * p.ext.size(), hipMemcpyHostToDevice));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  b->nq = nq;
  b->cls = p.cls;
  b->ran = false;
  return WSR_OK;
}
int wsr_batch_run(wsr_handle* h, wsr_batch* b) { return batch_run(h, b); }

// One run of the batch: plan, then the lean and general segment kernels on
// two streams; the worker that finishes a query's last item replays it
// (se == nullptr) or emits its reduced events into the owner's exchange
// region (a shard step).  Wide queries (k > kMaxK) of a plain run are
// replayed by one more launch after the segments.  oj: an earlier step
// group's owner replay for the lean kernel's tail (its exchange is done).
static std::atomic<int32_t> g_fail_runs{0};   // wsr_debug_fail_runs

int wsr_debug_fail_runs(int32_t n) {
  g_fail_runs.store(n > 0 ? n : 0);
  return WSR_OK;
}

}  // extern "C"

// What the kernels of a run of b do with a finished query: replay it into the
// batch's hit rows, or (se: a shard step) emit it into the exchange regions;
// oj: the owner replay the lean kernel's tail carries.
static FusedReplay fused_replay_of(const wsr_batch* b, const EmitView* se, const OwnerJob* oj) {
  FusedReplay fr{b->d_qdone, b->d_hits, b->stride, b->d_nhits};
  if (se) {
    fr.x_send = se->send;
    fr.x_meta = se->meta;
    fr.x_fill = b->d_ctr + kNumCounters;
    fr.x_err = b->d_ctr + kCtrError;
    fr.x_slot = se->slot;
    fr.x_stride = se->stride;
    fr.x_meta_stride = se->meta_stride;
    fr.x_qpr = se->qpr;
  }
  if (oj) fr.oj = *oj;
  return fr;
}

// (a shard step's callers have refused a batch with a disjunctive query: check_step, shard_exchange.cc)
int batch_run(wsr_handle* h, wsr_batch* b, const EmitView* se, const OwnerJob* oj) {
  if (!h || !b) return fail(WSR_E_INVALID, "null argument");
  const BatchClass& c = b->cls;
  for (int32_t f = g_fail_runs.load(); f > 0;)
    if (g_fail_runs.compare_exchange_weak(f, f - 1)) return fail(WSR_E_HIP, "injected run failure");
  wsr_batch* pb = nullptr;   // (a host replay taken, below)
  bool pb_queued = false;
  try {
    HIP_OK(hipSetDevice(h->device));
    hipStream_t st = b->st;
    // the previous shard step's exchange and owner replay (on the communicator's
    // stream) read this batch's buffers and write its results
    if (b->x.join()) HIP_OK(hipStreamWaitEvent(st, b->x.ev[1], 0));
    b->x.pending = false;
    // a host-exchange owner replay another batch deferred (wsr_shard_step_
    // replay_deferred) rides in this run's lean kernel, after its regions'
    // copy; its end is recorded on this stream behind the lean kernel
    OwnerJob hoj{};
    if (!oj && (pb = take_host_replay(h, b, &hoj))) {
      HIP_OK(hipStreamWaitEvent(st, pb->x.ev[0], 0));
      oj = &hoj;
    }
    HIP_OK(hipMemsetAsync(b->d_ctr, 0, sizeof(uint32_t) * (kNumCounters + (se ? se->owners : 0)), st));
    const FusedReplay fr = fused_replay_of(b, se, oj);
    HIP_OK(hipEventRecord(b->ev[0], st));
    IndexArgs pa = h->args;   // (the batch's item length)
    pa.seg_cap = b->seg_cap;
    // (which persistent kernels a batch with phrase queries launches: launches_of, batch_plan.h)
    b->launched = launches_of(c, se != nullptr, oj != nullptr);
    const bool run_conj = b->launched.conj, run_gen = b->launched.gen, run_tiny = b->launched.tiny;
    const int seg_grid = b->launched.gen_grid;   // (<= c.seg_grid, which places the statistics rows)
    HIP_OK(launch_plan(pa, b->d_q(), b->nq, b->d_plan, b->d_ctr, b->d_events.size(),
                       static_cast<uint32_t>(std::min<uint64_t>(b->d_evcnt.size(), 0xFFFFFFFFull)),
                       run_conj ? kLeanWaves * c.lean_wgs : 0,
                       c.has_phrase ? kLeanWaves * c.lean_wgs_ph : 0,
                       run_gen ? seg_grid : 0, b->launched.tiny_class ? c.n_tiny : -1, b->d_tinyq, fr, b->d_itemq, b->d_pub,
                       b->d_desc, b->d_part, st));
    HIP_OK(hipEventRecord(b->ev[1], st));
    // general items on the second stream, lean items here; both drain their
    // own queue, then the streams join
    HIP_OK(hipEventRecord(b->fork, st));
    HIP_OK(hipStreamWaitEvent(b->st2, b->fork, 0));
    if (run_gen)
      HIP_OK(launch_segments(h->args, b->d_q(), b->d_plan, b->nq, b->d_ctr, b->d_events, b->d_evcnt,
                             b->d_stats, seg_grid, fr, b->d_itemq, b->d_pub,
                             c.gen_phrase ? b->d_ph : nullptr, b->st2));
    // the tiny queries beside them: one wave each, results written in place
    if (run_tiny)
      HIP_OK(launch_tiny(h->args, b->d_q(), b->d_ctr, b->d_tinyq, static_cast<uint32_t>(b->max_q), c.n_tiny,
                         b->d_hits, b->stride, b->d_nhits, b->st2));
    uint32_t* lean_stats = b->d_stats + static_cast<size_t>(kStatStride) * c.seg_grid;
    HIP_OK(hipEventRecord(b->join, b->st2));
    if (c.has_phrase) {
      // The lean phrase queries' items run in the phrase instance (its
      // position check and registers) and the conjunctive lean items keep the
      // conjunctive instance's occupancy: the phrase launch on the batch
      // stream (where a phrase batch's lean kernel has always run, so that
      // consecutive batches' kernels rotate over the hardware queues as
      // before), the conjunctive one on the third stream beside it.  (A
      // deferred owner replay runs in the conjunctive launch only.)
      HIP_OK(hipStreamWaitEvent(b->st_pad, b->fork, 0));
      if (run_conj)
        HIP_OK(launch_lean(h->args, b->d_q(), b->d_plan, b->nq, b->d_ctr, b->d_events, b->d_evcnt, lean_stats,
                           c.lean_wgs, fr, b->d_itemq, b->d_pub, b->d_desc, false, c.two_conj, c.one_conj,
                           b->st_pad));
      if (pb) {   // the replay's end: behind the conjunctive launch that carried it
        HIP_OK(hipEventRecord(pb->x.ev[1], b->st_pad));
        pb_queued = true;
      }
      HIP_OK(hipEventRecord(b->join_ph, b->st_pad));
      FusedReplay frp = fr;
      frp.oj = OwnerJob{};
      HIP_OK(launch_lean(h->args, b->d_q(), b->d_plan, b->nq, b->d_ctr, b->d_events, b->d_evcnt,
                         lean_stats + static_cast<size_t>(kStatStride) * kLeanWaves * c.lean_wgs,
                         c.lean_wgs_ph, frp, b->d_itemq, b->d_pub, b->d_desc, true, c.two_ph, false, st));
    } else {
      HIP_OK(launch_lean(h->args, b->d_q(), b->d_plan, b->nq, b->d_ctr, b->d_events, b->d_evcnt, lean_stats,
                         c.lean_wgs, fr, b->d_itemq, b->d_pub, b->d_desc, false, c.two_conj, c.one_conj, st));
    }
    HIP_OK(hipEventRecord(b->ev[4], st));
    if (pb && !pb_queued) {
      HIP_OK(hipEventRecord(pb->x.ev[1], st));
      pb_queued = true;
    }
    if (pb) {
      pb->x.enqueued(true, false);   // (take_host_replay counted it in req)
      pb = nullptr;
    }
    HIP_OK(hipStreamWaitEvent(st, b->join, 0));
    if (c.has_phrase) HIP_OK(hipStreamWaitEvent(st, b->join_ph, 0));
    HIP_OK(hipEventRecord(b->ev[2], st));
    if (!se && c.has_wide)
      HIP_OK(launch_wide_replay(b->d_q(), b->d_plan, b->nq, b->d_events, b->d_evcnt, b->d_hits, b->stride,
                                b->d_nhits, st));
    if (c.n_or) {
      // the disjunctive queries, after the plan's writes of their (empty) rows
      HIP_OK(hipMemsetAsync(b->d_orstat, 0, sizeof(unsigned long long) * kNumOrStats, st));
      HIP_OK(launch_or_items(h->args, b->d_orq, b->d_oritem, c.or_items, c.or_nt_max, b->d_orev, b->d_orevcnt,
                             b->d_ctr, b->d_orstat, st));
      HIP_OK(launch_or_replay(b->d_orq, static_cast<uint32_t>(c.n_or), b->d_oritem, b->d_orev, b->d_orevcnt,
                              b->d_hits, b->stride, b->d_nhits, c.or_narrow, c.or_wide, st));
    }
    HIP_OK(hipEventRecord(b->ev[3], st));
  } catch (const std::exception& e) {
    if (pb) pb->x.enqueued(pb_queued || host_replay_enqueue(pb, h), false);   // (not queued: its own stream, then)
    return fail(WSR_E_HIP, e.what());
  }
  b->ran = true;
  b->x.fused = se != nullptr;
  return WSR_OK;
}

extern "C" {

int wsr_sync(wsr_handle* h) {
  if (!h) return fail(WSR_E_INVALID, "null argument");
  hipError_t e = hipSetDevice(h->device);
  if (e == hipSuccess) e = hipDeviceSynchronize();   // every batch's streams
  if (e != hipSuccess) return fail(WSR_E_HIP, hipGetErrorString(e));
  return WSR_OK;
}

// Results of the batch's last run: the counters, hit rows and hit counts go
// out as copies queued on the batch stream behind its kernels (and behind a
// shard step's exchange + owner replay), then one wait -- one host round trip
// instead of a synchronize per buffer (pinned destinations; pageable ones are
// copied after the wait).  The error flags are checked after the
// copies; on an error the output buffers hold whatever the run left and the
// call fails.  cols < stride copies the first cols entries of every row.
static bool host_pinned(const void* p) {
  if (!p) return true;
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();   // plain pageable memory: not an error of this call
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

static int batch_fetch(wsr_handle* h, wsr_batch* b, wsr_hit* hits, int32_t* n_hits, int32_t cols) {
  try {
    HIP_OK(hipSetDevice(h->device));
    hipStream_t st = b->st;
    if (b->x.join()) HIP_OK(hipStreamWaitEvent(st, b->x.ev[1], 0));   // a shard step's exchange + replay
    HIP_OK(hipMemcpyAsync(b->h_ctr, b->d_ctr, sizeof(uint32_t) * kNumCounters, hipMemcpyDeviceToHost, st));
    if (b->nq && !(host_pinned(hits) && host_pinned(n_hits))) {
      // pageable destinations: a queued copy into them is staged by the runtime
      // while the stream drains (serialising concurrent callers), so wait
      // first and copy after
      HIP_OK(hipStreamSynchronize(st));
      const uint32_t err = b->h_ctr[kCtrError];
      if (err) return fail(WSR_E_INTERNAL, "device reported error flags " + std::to_string(err));
      if (hits && cols == b->stride)
        HIP_OK(hipMemcpy(hits, b->d_hits, sizeof(HitDev) * b->nq * b->stride, hipMemcpyDeviceToHost));
      else if (hits)
        HIP_OK(hipMemcpy2D(hits, sizeof(HitDev) * cols, b->d_hits, sizeof(HitDev) * b->stride,
                           sizeof(HitDev) * cols, b->nq, hipMemcpyDeviceToHost));
      if (n_hits) HIP_OK(hipMemcpy(n_hits, b->d_nhits, sizeof(int32_t) * b->nq, hipMemcpyDeviceToHost));
      return WSR_OK;
    }
    if (b->nq) {
      if (hits && cols == b->stride)
        HIP_OK(hipMemcpyAsync(hits, b->d_hits, sizeof(HitDev) * b->nq * b->stride, hipMemcpyDeviceToHost, st));
      else if (hits)   // a pitched copy
        HIP_OK(hipMemcpy2DAsync(hits, sizeof(HitDev) * cols, b->d_hits, sizeof(HitDev) * b->stride,
                                sizeof(HitDev) * cols, b->nq, hipMemcpyDeviceToHost, st));
      if (n_hits)
        HIP_OK(hipMemcpyAsync(n_hits, b->d_nhits, sizeof(int32_t) * b->nq, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    const uint32_t err = b->h_ctr[kCtrError];
    if (err) return fail(WSR_E_INTERNAL, "device reported error flags " + std::to_string(err));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

int wsr_batch_fetch(wsr_handle* h, wsr_batch* b, wsr_hit* hits, int32_t* n_hits) {
  if (!h || !b || !b->ran) return fail(WSR_E_INVALID, "batch has not been run");
  return batch_fetch(h, b, hits, n_hits, b->stride);
}

int wsr_batch_fetch_cols(wsr_handle* h, wsr_batch* b, wsr_hit* hits, int32_t* n_hits, int32_t cols) {
  if (!h || !b || !b->ran) return fail(WSR_E_INVALID, "batch has not been run");
  if (cols < 1 || cols > b->stride) return fail(WSR_E_INVALID, "cols must be in [1, hit stride]");
  return batch_fetch(h, b, hits, n_hits, cols);
}

// (raw, not a PinnedBuf: the block's ownership crosses the C ABI to the caller)
int wsr_pinned_alloc(uint64_t bytes, void** out) {
  if (!out) return fail(WSR_E_INVALID, "null argument");
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, bytes ? bytes : 1);
  if (e != hipSuccess) return fail(WSR_E_HIP, hipGetErrorString(e));
  return WSR_OK;
}

void wsr_pinned_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int wsr_batch_ready(wsr_handle* h, wsr_batch* b) {
  if (!h || !b) return fail(WSR_E_INVALID, "null argument");
  if (!b->ran) return 0;
  hipError_t e = hipEventQuery(b->ev[3]);   // recorded after the batch's last kernel
  if (e == hipSuccess && b->x.join()) e = hipEventQuery(b->x.ev[1]);   // and a shard step's replay
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return fail(WSR_E_HIP, hipGetErrorString(e));
}

int wsr_batch_stats_get(wsr_handle* h, wsr_batch* b, wsr_batch_stats* out) {
  if (!h || !b || !out || !b->ran) return fail(WSR_E_INVALID, "batch has not been run");
  std::lock_guard<std::mutex> g(h->mu);
  try {
    HIP_OK(hipStreamSynchronize(b->st));
    if (b->x.join()) HIP_OK(hipEventSynchronize(b->x.ev[1]));   // a shard step's exchange + replay
    uint32_t ctr[kNumCounters];
    HIP_OK(hipMemcpy(ctr, b->d_ctr, sizeof ctr, hipMemcpyDeviceToHost));
    const int rows = b->cls.seg_grid + kLeanWaves * (b->cls.lean_wgs + (b->cls.has_phrase ? b->cls.lean_wgs_ph : 0));
    std::vector<uint32_t> ws(static_cast<size_t>(kStatStride) * rows);
    HIP_OK(hipMemcpy(ws.data(), b->d_stats, ws.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t sv = 0, db = 0, ob = 0, sk = 0;
    for (int i = 0; i < rows; ++i) {
      // (rows of a kernel the last run did not launch hold an earlier run's values)
      const bool conj_row = i >= b->cls.seg_grid && i < b->cls.seg_grid + kLeanWaves * b->cls.lean_wgs;
      if (i < b->cls.seg_grid ? !(b->launched.gen && i < b->launched.gen_grid) : (conj_row && !b->launched.conj))
        continue;
      // (the third word: a general workgroup's other-list blocks, a lean wave's skippable blocks)
      sv += ws[kStatStride * i]; db += ws[kStatStride * i + 1];
      (i < b->cls.seg_grid ? ob : sk) += ws[kStatStride * i + 2];
    }
    out->work_items = ctr[kCtrItems] + ctr[kCtrTiny];
    out->tiny_queries = ctr[kCtrTiny];
    // the tiny queries' matches (tiny_kernel keeps no statistics row: every match is scored and
    // handed to the heap, so it is a survivor and an event)
    uint64_t tiny_ev = 0, tiny_mx = 0;
    {
      const size_t nt = std::min<size_t>(ctr[kCtrTiny], static_cast<size_t>(b->max_q));
      std::vector<uint32_t> tc(nt);
      if (nt) HIP_OK(hipMemcpy(tc.data(), b->d_tinyq.get() + b->max_q, nt * sizeof(uint32_t), hipMemcpyDeviceToHost));
      for (uint32_t n : tc) { tiny_ev += n; tiny_mx = std::max<uint64_t>(tiny_mx, n); }
    }
    sv += tiny_ev;
    out->survivors = sv;
    out->driver_blocks = db;
    out->other_blocks = ob;
    out->skippable_blocks = sk;
    out->algo_bytes = b->cls.algo_static + sv;
    {
      const uint32_t items = ctr[kCtrItems];
      std::vector<uint32_t> ec(items);
      std::vector<QueryPlan> pl(b->nq);
      if (items) HIP_OK(hipMemcpy(ec.data(), b->d_evcnt, items * sizeof(uint32_t), hipMemcpyDeviceToHost));
      if (b->nq) HIP_OK(hipMemcpy(pl.data(), b->d_plan, pl.size() * sizeof(QueryPlan), hipMemcpyDeviceToHost));
      uint64_t tot = tiny_ev, mx = tiny_mx;
      for (const QueryPlan& p : pl) {
        uint64_t e = 0;
        for (uint32_t r = 0; r < p.n_items && p.item_base + r < items; ++r) e += ec[p.item_base + r];
        tot += e;
        mx = std::max(mx, e);
      }
      out->events = tot;
      out->max_query_events = mx;
    }
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, b->ev[0], b->ev[1])); out->plan_ms = ms;
    HIP_OK(hipEventElapsedTime(&ms, b->ev[1], b->ev[2])); out->segment_ms = ms;
    HIP_OK(hipEventElapsedTime(&ms, b->ev[2], b->ev[3])); out->replay_ms = ms;
    HIP_OK(hipEventElapsedTime(&ms, b->ev[1], b->ev[4])); out->lean_ms = ms;
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

int wsr_batch_or_stats_get(wsr_handle* h, wsr_batch* b, wsr_or_stats* out) {
  if (!h || !b || !out || !b->ran) return fail(WSR_E_INVALID, "batch has not been run");
  *out = wsr_or_stats{};
  if (!b->cls.n_or) return WSR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  try {
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(b->st));
    unsigned long long v[kNumOrStats];
    HIP_OK(hipMemcpy(v, b->d_orstat, sizeof v, hipMemcpyDeviceToHost));
    *out = or_stats_of(v);
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

int wsr_search_batch(wsr_handle* h, const wsr_query* q, int32_t nq, int32_t stride, wsr_hit* hits,
                     int32_t* n_hits) {
  if (!h || nq < 0 || (nq && (!q || !hits || !n_hits))) return fail(WSR_E_INVALID, "bad arguments");
  if (nq == 0) return WSR_OK;
  // batches are kept in a per-handle pool (one per concurrent caller): creating
  // one allocates its device buffers, which would dominate a small call
  wsr_batch* b = nullptr;
  {
    std::lock_guard<std::mutex> g(h->pool_mu);
    for (size_t i = 0; i < h->pool.size(); ++i)
      if (h->pool[i]->max_q >= nq && h->pool[i]->stride == stride) {
        b = h->pool[i];
        h->pool.erase(h->pool.begin() + i);
        break;
      }
  }
  if (!b) {
    int32_t cap = 64;
    while (cap < nq) cap *= 2;
    const int rc = wsr_batch_create(h, cap, stride, &b);
    if (rc) return rc;
  }
  int rc = wsr_batch_upload(h, b, q, nq);
  if (!rc) rc = wsr_batch_run(h, b);
  if (!rc) rc = wsr_batch_fetch(h, b, hits, n_hits);
  {
    std::lock_guard<std::mutex> g(h->pool_mu);
    if (!rc && h->pool.size() < 8) { h->pool.push_back(b); b = nullptr; }
  }
  if (b) wsr_batch_destroy(h, b);
  return rc;
}

int wsr_resolve_text(wsr_handle* h, const char* text, int64_t len, int32_t k, int32_t max_q,
                     wsr_query* q, int32_t* nq_out, int32_t* more_store, int64_t more_cap) {
  if (!h || (!text && len > 0) || len < 0 || max_q < 0 || (max_q && !q) || !nq_out || k < 0 ||
      more_cap < 0 || (more_cap > 0 && !more_store))
    return fail(WSR_E_INVALID, "bad resolve_text arguments");
  // QueryProducerByLog (query_pool.h:319-378): one query per line, terms
  // separated by spaces, a line in double quotes is a phrase query; each term
  // through the term index (VacuumInvertedIndex::FindIteratorsSolid,
  // vacuum_engine.h:89-99)
  int32_t n = 0;
  // the terms are parsed first and looked up together (find_many: the
  // dictionary's cache misses overlap)
  std::vector<const char*> tp;
  std::vector<uint32_t> tn;
  // (query, slot) of every parsed term; ids land in list_ids, or past 16 in
  // the caller's more_store (more_ids), once every term is looked up
  std::vector<std::pair<int32_t, int32_t>> dst;
  std::vector<size_t> more_at(static_cast<size_t>(max_q), 0);
  size_t n_more = 0;
  tp.reserve(static_cast<size_t>(max_q) * 2);
  tn.reserve(static_cast<size_t>(max_q) * 2);
  dst.reserve(static_cast<size_t>(max_q) * 2);
  for (int64_t at = 0; at < len;) {
    int64_t e = at;
    while (e < len && text[e] != '\n') ++e;
    int64_t a = at, z = e;
    at = e + 1;
    while (a < z && (text[a] == ' ' || text[a] == '\r' || text[a] == '\t')) ++a;
    while (z > a && (text[z - 1] == ' ' || text[z - 1] == '\r' || text[z - 1] == '\t')) --z;
    if (a == z) continue;
    if (n >= max_q) return fail(WSR_E_LIMIT, "more than max_q queries in the text");
    wsr_query& w = q[n];
    std::memset(&w, 0, sizeof w);
    if (z - a >= 2 && text[a] == '"' && text[z - 1] == '"') { w.flags = WSR_QUERY_PHRASE; ++a; --z; }
    w.k = k;
    more_at[n] = n_more;
    for (int64_t i = a; i < z;) {
      while (i < z && text[i] == ' ') ++i;
      int64_t j = i;
      while (j < z && text[j] != ' ') ++j;
      if (j > i) {
        if (w.n_terms >= WSR_MAX_QUERY_TERMS)
          return fail(WSR_E_LIMIT, "query " + std::to_string(n) + ": more than WSR_MAX_QUERY_TERMS terms");
        tp.push_back(text + i);
        tn.push_back(static_cast<uint32_t>(j - i));
        dst.emplace_back(n, w.n_terms++);
        if (w.n_terms > WSR_MAX_TERMS) ++n_more;
      }
      i = j;
    }
    for (int t = w.n_terms; t < WSR_MAX_TERMS; ++t) w.list_ids[t] = -1;
    ++n;
  }
  if (static_cast<int64_t>(n_more) > more_cap)
    return fail(WSR_E_LIMIT, "the text's queries need " + std::to_string(n_more) +
                                 " more_ids entries, more_store holds " + std::to_string(more_cap));
  std::vector<int32_t> ids(tp.size());
  h->idx.find_many(tp.data(), tn.data(), tp.size(), ids.data());
  for (size_t i = 0; i < ids.size(); ++i) {
    const int32_t qi = dst[i].first, slot = dst[i].second;
    if (slot < WSR_MAX_TERMS) q[qi].list_ids[slot] = ids[i];
    else more_store[more_at[qi] + (slot - WSR_MAX_TERMS)] = ids[i];
  }
  for (int32_t i = 0; i < n; ++i)
    if (q[i].n_terms > WSR_MAX_TERMS) q[i].more_ids = more_store + more_at[i];
  *nq_out = n;
  return WSR_OK;
}

int wsr_search_text(wsr_handle* h, const char* text, int64_t len, int32_t k, int32_t hit_stride,
                    int32_t max_q, wsr_hit* hits, int32_t* n_hits, int32_t* nq_out) {
  if (!h || !nq_out || max_q < 0) return fail(WSR_E_INVALID, "bad search_text arguments");
  std::vector<wsr_query> q(static_cast<size_t>(max_q));
  // (at most one more_ids entry per two text bytes: every term has a byte and
  // a separator; the ids are consumed within this call, so a per-thread
  // buffer is safe here)
  thread_local std::vector<int32_t> more;
  if (more.size() < static_cast<size_t>(len / 2 + 1)) more.resize(static_cast<size_t>(len / 2 + 1));
  int rc = wsr_resolve_text(h, text, len, k, max_q, q.data(), nq_out, more.data(),
                            static_cast<int64_t>(more.size()));
  if (rc) return rc;
  return wsr_search_batch(h, q.data(), *nq_out, hit_stride, hits, n_hits);
}

int wsr_class_order(const wsr_query* q, int32_t nq, int32_t* order, int32_t* n_conj) {
  if (nq < 0 || (nq && (!q || !order)) || !n_conj) return fail(WSR_E_INVALID, "bad class_order arguments");
  // (a one-term phrase is a single-term query: the same class as in the plan)
  // (a disjunctive query runs in kernels of its own: the last class)
  auto disj = [&](int32_t i) { return (q[i].flags & WSR_QUERY_OR) != 0; };
  auto phrase = [&](int32_t i) {
    return !disj(i) && (q[i].flags & WSR_QUERY_PHRASE) != 0 && q[i].n_terms > 1;
  };
  int32_t n = 0;
  for (int32_t i = 0; i < nq; ++i)
    if (!phrase(i) && !disj(i)) order[n++] = i;
  *n_conj = n;
  for (int32_t i = 0; i < nq; ++i)
    if (phrase(i)) order[n++] = i;
  for (int32_t i = 0; i < nq; ++i)
    if (disj(i)) order[n++] = i;
  return WSR_OK;
}

int wsr_shard_fill(wsr_handle* h, wsr_batch* b, int32_t n_owners, int64_t* owner_totals) {
  if (!h || !b || !b->x.fused || !owner_totals || n_owners <= 0 || n_owners > b->x.world)
    return fail(WSR_E_INVALID, "call wsr_shard_step (or wsr_shard_step_emit) first");
  try {
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(b->st));
    if (b->x.join()) HIP_OK(hipEventSynchronize(b->x.ev[1]));   // a shard step's exchange + replay
    // the segment kernels' per-owner fill counters
    std::vector<uint32_t> fill(n_owners);
    HIP_OK(hipMemcpy(fill.data(), b->d_ctr + kNumCounters, sizeof(uint32_t) * n_owners, hipMemcpyDeviceToHost));
    for (int i = 0; i < n_owners; ++i) owner_totals[i] = fill[i];
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

int wsr_batch_stream(wsr_handle* h, wsr_batch* b, void** stream) {
  if (!h || !b || !stream) return fail(WSR_E_INVALID, "null argument");
  *stream = b->st;
  return WSR_OK;
}

int wsr_batch_set_item_blocks(wsr_handle* h, wsr_batch* b, int32_t blocks) {
  if (!h || !b || blocks < 1 || blocks > kSegCost) return fail(WSR_E_INVALID, "item blocks must be 1..63");
  b->seg_cap = static_cast<uint32_t>(blocks);
  return WSR_OK;
}

int wsr_batch_stream_sync(wsr_handle* h, wsr_batch* b) {
  if (!h || !b) return fail(WSR_E_INVALID, "null argument");
  const hipError_t e = hipStreamSynchronize(b->st);
  return e == hipSuccess ? WSR_OK : fail(WSR_E_HIP, hipGetErrorString(e));
}

int wsr_batch_fetch_range(wsr_handle* h, wsr_batch* b, int32_t q0, int32_t nq, wsr_hit* hits,
                          int32_t* n_hits) {
  if (!h || !b || q0 < 0 || nq < 0 || q0 + nq > b->nq) return fail(WSR_E_INVALID, "bad range");
  try {
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(b->st));
    if (b->x.join()) HIP_OK(hipEventSynchronize(b->x.ev[1]));   // a shard step's exchange + replay
    uint32_t ctr[kNumCounters];
    HIP_OK(hipMemcpy(ctr, b->d_ctr, sizeof ctr, hipMemcpyDeviceToHost));
    if (ctr[kCtrError])
      return fail(WSR_E_INTERNAL, "device reported error flags " + std::to_string(ctr[kCtrError]) +
                                      (ctr[kCtrError] & kErrExchange ? " (an exchange slot overflowed)" : ""));
    if (nq && hits)
      HIP_OK(hipMemcpy(hits, b->d_hits + static_cast<size_t>(q0) * b->stride,
                       sizeof(HitDev) * static_cast<size_t>(nq) * b->stride, hipMemcpyDeviceToHost));
    if (nq && n_hits)
      HIP_OK(hipMemcpy(n_hits, b->d_nhits + q0, sizeof(int32_t) * nq, hipMemcpyDeviceToHost));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

int wsr_stream(wsr_handle* h, void** stream) {
  if (!h || !stream) return fail(WSR_E_INVALID, "null argument");
  *stream = h->stream;
  return WSR_OK;
}

int wsr_debug_decode_block(wsr_handle* h, int32_t id, int32_t block, int32_t which, uint32_t* out,
                           int32_t* count) {
  if (!h || !out || id < 0 || id >= static_cast<int32_t>(h->lists.size()))
    return fail(WSR_E_INVALID, "bad list id");
  const ListDev& L = h->lists[id];
  if (block < 0 || static_cast<uint32_t>(block) >= L.nblk) return fail(WSR_E_INVALID, "bad block");
  std::lock_guard<std::mutex> g(h->mu);
  const BlockDev& bd = h->blocks[L.blk0 + block];
  const uint32_t cnt = static_cast<uint32_t>(block) == L.nblk - 1 ? L.tail_cnt : 128u;
  try {
    gpu::DevBuf<uint32_t> d_out;
    d_out.alloc(128);
    const uint8_t* p = h->d_blob.get() + L.base + (which ? bd.tf_rel : bd.doc_rel);
    const uint32_t bits = which ? (h->meta[L.blk0 + block] >> 8) : (h->meta[L.blk0 + block] & 0xFF);
    HIP_OK(launch_decode_probe(p, bits, cnt, which == 0, bd.prev, d_out, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    HIP_OK(hipMemcpy(out, d_out, d_out.bytes(), hipMemcpyDeviceToHost));
  } catch (const std::exception& ex) {
    return fail(WSR_E_HIP, ex.what());
  }
  if (count) *count = static_cast<int32_t>(cnt);
  return WSR_OK;
}

int wsr_debug_wg_stats(wsr_handle* h, wsr_batch* b, uint32_t* out, int32_t max_words,
                       int32_t* n_wg, int32_t* stride) {
  if (!h || !b) return fail(WSR_E_INVALID, "null argument");
  std::lock_guard<std::mutex> g(h->mu);
  // general workgroups, then lean waves (the conjunctive instance's, then the phrase instance's);
  // the rows of a kernel the last run did not launch (b->launched) are stale
  const int rows = b->cls.seg_grid + kLeanWaves * (b->cls.lean_wgs + (b->cls.has_phrase ? b->cls.lean_wgs_ph : 0));
  if (n_wg) *n_wg = rows;
  if (stride) *stride = kStatStride;
  if (!out) return WSR_OK;
  const size_t n = std::min<size_t>(static_cast<size_t>(std::max(max_words, 0)),
                                    static_cast<size_t>(kStatStride) * rows);
  try {
    HIP_OK(hipStreamSynchronize(b->st));
    if (b->x.join()) HIP_OK(hipEventSynchronize(b->x.ev[1]));   // a shard step's exchange + replay
    HIP_OK(hipMemcpy(out, b->d_stats, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

int wsr_debug_batch_class(wsr_handle* h, wsr_batch* b, uint32_t* flags) {
  if (!h || !b || !flags) return fail(WSR_E_INVALID, "null argument");
  const BatchClass& c = b->cls;
  *flags = (c.two_conj ? WSR_CLASS_TWO_CONJ : 0u) | (c.one_conj ? WSR_CLASS_ONE_CONJ : 0u) |
           (c.has_phrase ? WSR_CLASS_HAS_PHRASE : 0u) | (c.two_ph ? WSR_CLASS_TWO_PH : 0u) |
           (c.has_wide ? WSR_CLASS_HAS_WIDE : 0u) | (c.gen_phrase ? WSR_CLASS_GEN_PHRASE : 0u) |
           (c.has_conj_lean ? WSR_CLASS_HAS_CONJ_LEAN : 0u) | (c.has_gen ? WSR_CLASS_HAS_GEN : 0u) |
           (c.has_or ? WSR_CLASS_HAS_OR : 0u) | (b->launched.conj ? WSR_CLASS_RAN_CONJ : 0u) |
           (b->launched.gen ? WSR_CLASS_RAN_GEN : 0u);
  return WSR_OK;
}

int wsr_debug_dense_lookup(const char* dir, uint32_t doc_lo, uint32_t doc_hi, uint32_t dense_div,
                           const char* term, const uint32_t* docs, int32_t n, int32_t* tf_out,
                           int32_t* is_dense) {
  if (!dir || !term || (n > 0 && (!docs || !tf_out))) return fail(WSR_E_INVALID, "null argument");
  try {
    VacuumIndex idx;
    idx.open(dir);
    const HostImage img = build_image(idx, doc_lo, doc_hi ? doc_hi : 0xFFFFFFFFu, 4, dense_div);
    const int32_t id = idx.find(term);
    const bool dense = id >= 0 && img.lists[id].bm != kNoDense;
    if (is_dense) *is_dense = dense ? 1 : 0;
    for (int32_t i = 0; i < n; ++i)
      tf_out[i] = dense ? static_cast<int32_t>(dense_lookup_host(img, img.lists[id], docs[i])) : -1;
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_debug_doc16(const char* dir, uint32_t doc_lo, uint32_t doc_hi, const char* term, int32_t max_blocks,
                    uint16_t* out, uint32_t* prev, int32_t* n_blocks, int32_t* eligible, int32_t* probe) {
  if (!dir || !term || !n_blocks || !eligible || !probe || max_blocks < 0 || (max_blocks > 0 && (!out || !prev)))
    return fail(WSR_E_INVALID, "bad argument");
  try {
    VacuumIndex idx;
    idx.open(dir);
    const HostImage img = build_image(idx, doc_lo, doc_hi ? doc_hi : 0xFFFFFFFFu, 4, dense_div_knob(), false,
                                      dense_budget_knob(), false, 0, doc16_knob());
    const int32_t id = idx.find(term);
    if (id < 0) return fail(WSR_E_INVALID, "no such term");
    const ListDev& L = img.lists[id];
    *n_blocks = static_cast<int32_t>(L.nblk);
    *probe = L.bm == kNoDense ? -1 : static_cast<int32_t>(probe_shift(L.bm));
    *eligible = !img.d16_blk.empty() && img.d16_blk[id] != kNoDoc16;
    for (uint32_t b = 0; b < L.nblk && b < static_cast<uint32_t>(max_blocks); ++b) {
      prev[b] = img.blocks[L.blk0 + b].prev;
      if (*eligible)
        std::memcpy(out + 128ull * b, &img.doc16[(static_cast<uint64_t>(img.d16_blk[id]) + b) * 128],
                    128 * sizeof(uint16_t));
    }
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_doc16_survey(const char* dir, const char* const* terms, int32_t n, uint32_t* n_blocks,
                     uint32_t* pack_blocks, uint32_t* ok_blocks, int32_t* eligible) {
  if (!dir || (n > 0 && (!terms || !n_blocks || !pack_blocks || !ok_blocks || !eligible)))
    return fail(WSR_E_INVALID, "null argument");
  try {
    VacuumIndex idx;
    idx.open(dir);
    for (int32_t i = 0; i < n; ++i) {
      const int32_t id = terms[i] ? idx.find(terms[i]) : -1;
      n_blocks[i] = pack_blocks[i] = ok_blocks[i] = 0;
      bool ok = false;
      if (id >= 0) doc16_survey(idx, id, &n_blocks[i], &pack_blocks[i], &ok_blocks[i], &ok);
      eligible[i] = ok ? 1 : 0;
    }
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

// ------------------------------------------------------------ building --
static void fill_stats(const BuildStats& s, wsr_build_stats* st) {
  if (!st) return;
  st->n_docs = s.n_docs;
  st->n_terms = s.n_terms;
  st->n_postings = s.n_postings;
  st->vacuum_bytes = s.vacuum_bytes;
  st->docs_char4_ge_0x80 = s.docs_char4_ge_0x80;
  st->avg_length = s.avg_length;
}

int wsr_build_from_linedoc(const char* linedoc, int64_t n_rows, const char* format,
                           const char* out_dir, wsr_build_stats* st) {
  if (!linedoc || !format || !out_dir) return fail(WSR_E_INVALID, "null argument");
  try {
    fill_stats(build_from_linedoc(linedoc, n_rows, format, out_dir), st);
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_build_from_linedoc_bloom(const char* linedoc, int64_t n_rows, const char* format,
                                 const char* out_dir, float ratio, int32_t expected_entries,
                                 wsr_build_stats* st) {
  if (!linedoc || !format || !out_dir) return fail(WSR_E_INVALID, "null argument");
  if (!(ratio > 0.0f && ratio < 1.0f) || expected_entries < 1)
    return fail(WSR_E_INVALID, "bloom ratio must be in (0, 1) and expected entries >= 1");
  try {
    BloomSpec b;
    b.on = true;
    b.ratio = ratio;
    b.entries = expected_entries;
    fill_stats(build_from_linedoc(linedoc, n_rows, format, out_dir, b), st);
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_build_synthetic(const char* out_dir, int64_t n_docs, int64_t vocab, double zipf_s,
                        uint64_t seed, int32_t with_positions, int32_t threads,
                        wsr_build_stats* st) {
  if (!out_dir || n_docs <= 0 || vocab <= 0) return fail(WSR_E_INVALID, "bad arguments");
  try {
    SyntheticSpec sp;
    sp.n_docs = n_docs;
    sp.vocab = vocab;
    sp.zipf_s = zipf_s;
    sp.seed = seed;
    sp.with_positions = with_positions != 0;
    sp.threads = threads;
    fill_stats(build_synthetic(sp, out_dir), st);
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_build_wiki_standin(const char* out_dir, int64_t n_docs, double term_scale, uint64_t seed,
                           int32_t threads, wsr_build_stats* st) {
  if (!out_dir || n_docs < 16 || !(term_scale > 0)) return fail(WSR_E_INVALID, "bad arguments");
  try {
    WikiSpec sp;
    sp.n_docs = n_docs;
    sp.term_scale = term_scale;
    sp.seed = seed;
    sp.threads = threads;
    fill_stats(build_wiki_standin(sp, out_dir), st);
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_build_wiki_standin_topics(const char* out_dir, int64_t n_docs, double term_scale, uint64_t seed,
                                  int32_t threads, int32_t topics, int32_t topics_per_term, double affinity,
                                  wsr_build_stats* st) {
  if (!out_dir || n_docs < 16 || !(term_scale > 0) || topics < 1 || topics_per_term < 1 || topics_per_term > 16 ||
      !(affinity >= 0 && affinity <= 1) || topics > n_docs)
    return fail(WSR_E_INVALID, "bad arguments");
  try {
    WikiSpec sp;
    sp.n_docs = n_docs;
    sp.term_scale = term_scale;
    sp.seed = seed;
    sp.threads = threads;
    sp.topics = topics;
    sp.topics_per_term = topics_per_term;
    sp.affinity = affinity;
    fill_stats(build_wiki_standin(sp, out_dir), st);
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_gen_two_term_log(const char* index_dir, int64_t n_queries, uint64_t seed,
                         const char* out_path, int64_t* n_written) {
  if (!index_dir || !out_path) return fail(WSR_E_INVALID, "null argument");
  try {
    int64_t n = gen_two_term_log(index_dir, n_queries, seed, out_path);
    if (n_written) *n_written = n;
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_gen_mixed_log(const char* index_dir, int64_t n_queries, uint64_t seed,
                      const char* out_path, int64_t* n_written) {
  if (!index_dir || !out_path) return fail(WSR_E_INVALID, "null argument");
  try {
    int64_t n = gen_mixed_log(index_dir, n_queries, seed, out_path);
    if (n_written) *n_written = n;
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_gen_single_term_log(const char* index_dir, int32_t high, int64_t n_queries, uint64_t seed,
                      const char* out_path, int64_t* n_written) {
  if (!index_dir || !out_path) return fail(WSR_E_INVALID, "null argument");
  try {
    int64_t n = gen_single_term_log(index_dir, high != 0, n_queries, seed, out_path);
    if (n_written) *n_written = n;
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

int wsr_gen_phrase_log(const char* index_dir, int64_t n_queries, uint64_t seed,
                       const char* out_path, int64_t* n_written) {
  if (!index_dir || !out_path) return fail(WSR_E_INVALID, "null argument");
  try {
    int64_t n = gen_phrase_log(index_dir, n_queries, seed, out_path);
    if (n_written) *n_written = n;
  } catch (const std::exception& e) {
    return fail(WSR_E_IO, e.what());
  }
  return WSR_OK;
}

}  // extern "C"
