// Doc-range shard steps of the C ABI (include/wiser_hip.h): step groups over a
// communicator (RCCL, or the loopback group of one process), the
// communicator's exchange worker, the host-exchange halves, and the owner
// replays deferred into later lean kernels.  The regions' layout and the two
// device views of it: shard_layout.h.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <thread>

#include "engine_impl.h"

using namespace wiser;

// ---- native RCCL exchange (one process per GPU, no Python in the loop) ----
// Every collective of a communicator runs on its one stream, in issue order
// (the same order on every rank), whatever batch stream it serves: a step's
// pack is joined into it by an event and its replay waits for it by another,
// so consecutive batches still overlap their kernels.
// The exchange half of a step group (the collective and the owner replays)
// is enqueued by the communicator's own worker thread: an ncclAllToAll call
// can hold its caller for milliseconds while the device is busy (RCCL's host
// side waits for its earlier work: 0.13-0.23 ms of host time per step in the
// hybrid rehearsal, the loop host-bound, profiles/r04g/), and the caller's
// next batches must not wait behind it.  Jobs run in submission order, so
// every rank issues its collectives in the same order.
//
// A group's owner replays are deferred (WSR_REPLAY_DEFER, default 1) into the
// lean kernels of the step group kReplayLag groups later: each of its
// batches' lean kernel, its own items done, replays one batch of the earlier
// group (OwnerJob).  A separate owner replay launch -- thousands of one-wave,
// latency-bound workgroups per batch beside the persistent lean kernels --
// cost more than its work (one-rank rehearsal 16.8 M q/s with it, 20.9 M with
// the replay dropped, profiles/r04r/).  Whatever needs a deferred replay's
// results first (a fetch, the batch's next run, wsr_comm_flush) enqueues it
// on the communicator's stream instead (replay_flush).
struct XGroup {
  XGroup(wsr_handle* h_, wsr_batch* const* bs_, int32_t n, int32_t qpr, int64_t slot, int xs_, bool defer_)
      : h(h_), bs(bs_, bs_ + n), layout(qpr, slot, static_cast<uint64_t>(n)), xs(xs_), defer(defer_),
        queued(static_cast<size_t>(n), defer_ ? 0 : 1) {}
  wsr_handle* h;
  std::vector<wsr_batch*> bs;
  ShardLayout layout;                  // batch i's regions at batch_at(i) of every owner's run
  int xs;                              // its exchange buffers: c->xs[xs]
  bool defer;
  std::vector<hipEvent_t> wait_done;   // the slot's previous replays (before the all-to-all)
  std::vector<uint8_t> queued;         // deferred: bs[i]'s replay enqueued
  std::atomic<bool> enq{false};        // the worker has enqueued the all-to-all (and, not deferred, the replays)
};
using XJob = std::shared_ptr<XGroup>;
constexpr int kXSlots = 4;       // exchange buffer sets in rotation
constexpr size_t kReplayLag = 2;  // groups between a group's exchange and its deferred replays
struct XSlot {
  gpu::DevBuf<Event> send, recv;
  gpu::Event xa;                      // the last all-to-all out of this slot done (comm stream)
  std::vector<gpu::Event> done;       // its group's owner replays done, one per batch
  size_t n_done = 0;                  // (recorded)
  std::shared_ptr<XGroup> last;       // the group that used it last
};
// Loopback group (wsr_loopback_create): the all-to-all of W communicators of
// one process by device copies.  Call n of every rank meets in calls[n]:
// each rank records its send buffer ready, waits on the host until all W have
// (phase 1), copies region r of every rank's send buffer into slot g of its
// receive buffer behind that rank's ready event, records its reads done and
// waits until all W have (phase 2), then makes its stream wait for every
// rank's reads -- so a rank's collective completes only once its send buffer
// has been read by all, as ncclAllToAll's does, and no rank records its
// per-communicator events again before every rank has waited on them.
struct wsr_loopback {
  int world = 0;
  std::mutex mu;
  std::condition_variable cv;
  struct Call {
    std::vector<const void*> send;
    std::vector<hipEvent_t> ready, read;
    int arrived = 0, read_done = 0, left = 0;
  };
  std::map<uint64_t, Call> calls;
};

struct wsr_comm {
  ncclComm_t comm = nullptr;
  wsr_loopback* loop = nullptr;   // a loopback communicator (no RCCL)
  uint64_t loop_seq = 0;
  gpu::Event loop_ready, loop_read;
  gpu::Stream stream;
  int world = 0, rank = 0, device = 0;
  // WSR_HOST_TIMING=1: host time per phase of wsr_shard_step (enqueue only),
  // printed to stderr when the communicator closes
  bool timing = false;
  uint64_t steps = 0, t_ns[4] = {0, 0, 0, 0};   // run, submit, rccl (worker), replay (worker)
  std::thread worker;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<XJob> jobs;   // (FIFO)
  size_t head = 0;
  bool stop = false;
  std::atomic<int> err{WSR_OK};   // the worker's first failure, reported by the next call
  std::string err_msg;
  XSlot xs[kXSlots];
  uint64_t n_groups = 0;
  std::atomic<int64_t> replays_lean{0}, replays_stream{0};   // wsr_comm_stats
  bool defer = true;
  // deferred groups, oldest first.  pend, XGroup::queued and the batches'
  // x.comm are changed by wsr_shard_steps and by whatever flushes a deferred
  // replay (a join inside a fetch, upload, run or destroy; wsr_comm_flush),
  // which may run on other threads: pend_mu orders them (recursive: a step
  // group flushes its own batches' earlier replays).
  std::deque<std::shared_ptr<XGroup>> pend;
  std::recursive_mutex pend_mu;
};

static void replay_flush(wsr_comm* c, const wsr_batch* upto);
static void host_replay_flush(wsr_batch* b);

bool ShardExchange::join() {
  if (hdef) host_replay_flush(batch);
  if (wsr_comm* c = comm.load(std::memory_order_acquire)) replay_flush(c, batch);
  while (enq.load(std::memory_order_acquire) != req.load(std::memory_order_acquire)) std::this_thread::yield();
  return pending;
}

static void set_comm_err(wsr_comm* c, int rc, const std::string& msg) {
  std::lock_guard<std::mutex> g(c->mu);
  if (c->err.load() == WSR_OK) {
    c->err_msg = msg;
    c->err.store(rc);
  }
}

static uint64_t now_ns() {
  return static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                   std::chrono::steady_clock::now().time_since_epoch())
                                   .count());
}

// The loopback group's all-to-all (wsr_loopback above): bytes per rank pair.
static void loopback_alltoall(wsr_comm* c, const Event* send, Event* recv, uint64_t bytes) {
  wsr_loopback* L = c->loop;
  const int W = L->world, r = c->rank;
  HIP_OK(hipEventRecord(c->loop_ready, c->stream));
  const uint64_t n = c->loop_seq++;
  wsr_loopback::Call* call;
  {
    std::unique_lock<std::mutex> lk(L->mu);
    call = &L->calls[n];
    if (call->send.empty()) {
      call->send.assign(W, nullptr);
      call->ready.assign(W, nullptr);
      call->read.assign(W, nullptr);
    }
    call->send[r] = send;
    call->ready[r] = c->loop_ready;
    ++call->arrived;
    L->cv.notify_all();
    L->cv.wait(lk, [&] { return call->arrived == W; });
  }
  const uint8_t* src_base = nullptr;
  for (int g = 0; g < W; ++g) {
    HIP_OK(hipStreamWaitEvent(c->stream, call->ready[g], 0));
    src_base = static_cast<const uint8_t*>(call->send[g]);
    HIP_OK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(recv) + g * bytes, src_base + r * bytes, bytes,
                          hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_OK(hipEventRecord(c->loop_read, c->stream));
  {
    std::unique_lock<std::mutex> lk(L->mu);
    call->read[r] = c->loop_read;
    ++call->read_done;
    L->cv.notify_all();
    L->cv.wait(lk, [&] { return call->read_done == W; });
  }
  for (int g = 0; g < W; ++g) HIP_OK(hipStreamWaitEvent(c->stream, call->read[g], 0));
  {
    std::lock_guard<std::mutex> lk(L->mu);
    if (++call->left == W) L->calls.erase(n);
  }
}

// The owner replay of this rank's queries of b over batch `index` of the
// receive buffer at base (run g of it: what shard g sent this owner).
static OwnerJob owner_job_of(const wsr_batch* b, const Event* base, const ShardLayout& l, uint64_t index, int rank,
                             int world) {
  OwnerJob of{};
  of.qs = b->d_q();
  of.hits = b->d_hits;
  of.n_hits = b->d_nhits;
  of.counters = b->d_ctr;
  of.hit_stride = b->stride;
  return owner_job_of(of, base, l, index, rank, world);
}

// ... as a launch of its own on st
static int owner_replay_on(wsr_handle* h, const wsr_batch* b, const OwnerJob& oj, hipStream_t st) {
  try {
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(launch_owner_replay(oj, b->cls.has_wide, st));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

// ... of a batch's last emission into its own buffers (wsr_shard_step_emit)
static int own_replay_on(wsr_handle* h, const wsr_batch* b, int rank, hipStream_t st) {
  return owner_replay_on(h, b, owner_job_of(b, b->x.recv, b->x.layout(), 0, rank, b->x.world), st);
}

// The end of b's owner replay on st: its own event and its exchange slot's.
static bool record_replay_end(wsr_batch* b, hipEvent_t slot_done, hipStream_t st) {
  return hipEventRecord(b->x.ev[1], st) == hipSuccess && hipEventRecord(slot_done, st) == hipSuccess;
}

// The owner replay of batch i of group g on the communicator's stream (after
// the group's all-to-all), and its end.
static int group_replay_on_stream(wsr_comm* c, const XGroup& g, size_t i) {
  const XSlot& S = c->xs[g.xs];
  wsr_batch* b = g.bs[i];
  if (int rc = owner_replay_on(g.h, b, owner_job_of(b, S.recv, g.layout, i, c->rank, c->world), c->stream))
    return rc;
  return record_replay_end(b, S.done[i], c->stream) ? WSR_OK : fail(WSR_E_HIP, "hipEventRecord failed");
}

// One job: wait for the group's emissions (and for the slot's previous
// replays), one ncclAllToAll of the owners' runs of regions, then -- not
// deferred -- the owner replays and the end event of every batch.
static void run_xjob(wsr_comm* c, const XJob& jp) {
  XGroup& j = *jp;
  XSlot& S = c->xs[j.xs];
  const uint64_t run = j.layout.run();
  uint64_t t0 = c->timing ? now_ns() : 0;
  int rc = WSR_OK;
  std::string msg;
  try {
    HIP_OK(hipSetDevice(c->device));
    // (the device waits for the emissions, not this thread: waiting on the
    // host first makes the collective's own call short, 2-8 us, but the loop
    // no faster -- the enqueueing thread is held by full hardware queues
    // either way, and the exchange starts later: 16.8 -> 15.3 M q/s every
    // query sharded, profiles/r04t/)
    for (wsr_batch* b : j.bs) HIP_OK(hipStreamWaitEvent(c->stream, b->x.ev[0], 0));
    for (hipEvent_t e : j.wait_done) HIP_OK(hipStreamWaitEvent(c->stream, e, 0));
    if (c->loop) {
      loopback_alltoall(c, S.send, S.recv, ShardLayout::bytes(run));
    } else {
      const ncclResult_t r = ncclAllToAll(S.send, S.recv, run * (sizeof(Event) / sizeof(uint64_t)),
                                          ncclUint64, c->comm, c->stream);
      if (r != ncclSuccess) throw std::runtime_error(std::string("ncclAllToAll: ") + ncclGetErrorString(r));
    }
    HIP_OK(hipEventRecord(S.xa, c->stream));
  } catch (const std::exception& e) {
    rc = WSR_E_HIP;
    msg = e.what();
  }
  uint64_t t1 = c->timing ? now_ns() : 0;
  if (!j.defer) {
    for (size_t i = 0; i < j.bs.size() && rc == WSR_OK; ++i)
      if ((rc = group_replay_on_stream(c, j, i))) msg = g_err;
    for (wsr_batch* b : j.bs) b->x.enqueued(rc == WSR_OK, false);
    c->replays_stream.fetch_add(static_cast<int64_t>(j.bs.size()));
  }
  if (rc != WSR_OK) set_comm_err(c, rc, msg);
  j.enq.store(true, std::memory_order_release);
  if (c->timing) {
    const uint64_t t2 = now_ns();
    c->t_ns[2] += t1 - t0;
    c->t_ns[3] += t2 - t1;
  }
}

static void exchange_worker(wsr_comm* c) {
  for (;;) {
    XJob j;
    {
      std::unique_lock<std::mutex> lk(c->mu);
      c->cv.wait(lk, [&] { return c->stop || c->head < c->jobs.size(); });
      if (c->head == c->jobs.size()) return;   // (stop, and drained)
      j = std::move(c->jobs[c->head++]);
      if (c->head == c->jobs.size()) {
        c->jobs.clear();
        c->head = 0;
      }
    }
    run_xjob(c, j);
  }
}

// The events that order a shard step's exchange against the batch's runs.
static void ensure_xev(wsr_batch* b) {
  for (auto& e : b->x.ev) if (!e) e = gpu::make_event();
}

// The exchange buffers of b: send and receive, need events each.
static void ensure_xbuf(wsr_batch* b, uint64_t need, int W) {
  if (need > b->x.send.size() || W != b->x.pairs) {
    if (b->x.join()) HIP_OK(hipEventSynchronize(b->x.ev[1]));
    gpu::alloc_group(need, b->x.send, b->x.recv);
    b->x.pairs = W;
  }
  ensure_xev(b);
}

extern "C" {

int wsr_comm_unique_id(uint8_t* id) {
  if (!id) return fail(WSR_E_INVALID, "null argument");
  ncclUniqueId u;
  const ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) return fail(WSR_E_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  static_assert(sizeof(ncclUniqueId) == WSR_COMM_ID_BYTES, "RCCL unique id size");
  std::memcpy(id, &u, sizeof u);
  return WSR_OK;
}

// The tail of both opens: the communicator's place, its deferral knob and its worker.
static wsr_comm* start_comm(std::unique_ptr<wsr_comm> c, int32_t world, int32_t rank, int32_t device) {
  c->world = world;
  c->rank = rank;
  c->device = device;
  c->defer = env_number("WSR_REPLAY_DEFER", 1) != 0;
  wsr_comm* cp = c.release();
  cp->worker = std::thread([cp] { exchange_worker(cp); });
  return cp;
}

int wsr_comm_open(const uint8_t* id, int32_t world, int32_t rank, int32_t device, wsr_comm** out) {
  if (!id || !out || world < 1 || rank < 0 || rank >= world) return fail(WSR_E_INVALID, "bad comm arguments");
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return fail(WSR_E_HIP, "hipSetDevice failed");
  std::unique_ptr<wsr_comm> c(new wsr_comm());
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  const ncclResult_t r = ncclCommInitRank(&c->comm, world, u, rank);
  if (r != ncclSuccess) return fail(WSR_E_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  // exchange stream priority (WSR_COMM_PRIORITY=1: high).  Normal since
  // round 4: at high priority the owner replays' thousands of one-wave
  // workgroups are dispatched ahead of the next batches' persistent kernels;
  // one-rank rehearsal 15.6 -> 16.7 M q/s every query sharded, 12.7 -> 15.4 M
  // hybrid (profiles/r04g/; round 2 had measured +3 % for high)
  // (a stream with a full CU mask, i.e. a hardware queue of its own at normal
  // priority, was slower again: 16.5 / 14.2 M against 17.0 / 15.6 M,
  // profiles/r04n/; low priority was slower still: 16.3 / 12.9 M against
  // 16.7 / 15.3 M, profiles/r04s/)
  int lo_prio = 0, hi_prio = 0;
  const bool prio = env_number("WSR_COMM_PRIORITY", 0) != 0 &&
                    hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio) == hipSuccess;
  try {
    c->stream = gpu::make_stream(prio ? &hi_prio : nullptr);
  } catch (const std::exception& e) {
    (void)ncclCommDestroy(c->comm);
    return fail(WSR_E_HIP, e.what());
  }
  const char* ht = std::getenv("WSR_HOST_TIMING");
  c->timing = ht && *ht && *ht != '0';
  *out = start_comm(std::move(c), world, rank, device);
  return WSR_OK;
}

int wsr_loopback_create(int32_t world, wsr_loopback** out) {
  if (!out || world < 1 || world > kMaxOwners) return fail(WSR_E_INVALID, "bad loopback arguments");
  *out = new wsr_loopback();
  (*out)->world = world;
  return WSR_OK;
}

void wsr_loopback_destroy(wsr_loopback* l) { delete l; }

int wsr_comm_open_loopback(wsr_loopback* l, int32_t rank, int32_t device, wsr_comm** out) {
  if (!l || !out || rank < 0 || rank >= l->world) return fail(WSR_E_INVALID, "bad loopback comm arguments");
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return fail(WSR_E_HIP, "hipSetDevice failed");
  std::unique_ptr<wsr_comm> c(new wsr_comm());
  c->loop = l;
  try {
    c->stream = gpu::make_stream();
    c->loop_ready = gpu::make_event();
    c->loop_read = gpu::make_event();
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  *out = start_comm(std::move(c), l->world, rank, device);
  return WSR_OK;
}

void wsr_comm_close(wsr_comm* c) {
  if (!c) return;
  (void)wsr_comm_flush(c);   // (every deferred replay enqueued before the worker stops)
  {
    std::lock_guard<std::mutex> g(c->mu);
    c->stop = true;
  }
  c->cv.notify_one();
  if (c->worker.joinable()) c->worker.join();
  if (c->timing && c->steps)
    std::fprintf(stderr, "wsr_shard_step host us/step over %llu steps: run %.1f submit %.1f rccl %.1f replay %.1f "
                 "(rccl and replay: the exchange worker)\n",
                 static_cast<unsigned long long>(c->steps), c->t_ns[0] / 1e3 / c->steps,
                 c->t_ns[1] / 1e3 / c->steps, c->t_ns[2] / 1e3 / c->steps, c->t_ns[3] / 1e3 / c->steps);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (XSlot& S : c->xs)
    for (size_t i = 0; i < S.n_done; ++i) (void)hipEventSynchronize(S.done[i]);   // (replays in lean kernels)
  if (c->comm) (void)ncclCommDestroy(c->comm);   // (ahead of its stream, which goes with c)
  delete c;
}

}  // extern "C"

// One step of a doc-range sharded batch, all of it enqueued, nothing waited on:
//   batch stream: the plan + segment kernels; the worker that finishes a
//     query reduces its events into the owner's region of the send buffer;
//   communicator stream (joined by x.ev[0]): one ncclAllToAll of the regions
//     (RCCL's pairwise exchange over xGMI), then the owner replay of this
//     rank's queries; x.ev[1] marks the end.
// An owner's region holds its queries' {count, offset} pairs and its slot
// (ShardLayout), so one collective moves both.  The batch stream
// never waits on the exchange inside a step, so the next batches' kernels run
// under it; the next run of this batch waits for x.ev[1] (long past by then),
// and the fetches join it.
static int check_step(wsr_handle* h, wsr_batch* b, int W, int32_t q_per_owner, int64_t slot) {
  if (!h || !b || W < 1 || q_per_owner <= 0 || slot <= 0 || static_cast<int64_t>(q_per_owner) * W != b->nq)
    return fail(WSR_E_INVALID, "bad shard_step arguments (the batch must hold world * q_per_owner queries)");
  if (b->cls.has_or) return fail(WSR_E_INVALID, "a doc-range shard step cannot run a disjunctive query");
  if (W > kMaxOwners) return fail(WSR_E_LIMIT, "more than kMaxOwners ranks");
  if (static_cast<uint64_t>(slot) > 0xFFFFFFFFull) return fail(WSR_E_LIMIT, "slot over 2^32 events");
  return WSR_OK;
}

// First half of a shard step: run the batch with fused emission into its
// regions (batch `index` of l) of the send buffer at base: its own buffer, or
// a step group's.
static int step_emit_into(wsr_handle* h, wsr_batch* b, int W, const ShardLayout& l, Event* base, uint64_t index,
                          const OwnerJob* oj = nullptr) {
  const EmitView se = emit_view_of(base, l, index, W);
  const int rc = batch_run(h, b, &se, oj);
  if (rc == WSR_OK) {
    b->x.world = W;
    b->x.qpr = l.qpr;
    b->x.slot = static_cast<int64_t>(l.slot);
  }
  return rc;
}

static int step_emit(wsr_handle* h, wsr_batch* b, int W, int32_t q_per_owner, int64_t slot) {
  if (int rc = check_step(h, b, W, q_per_owner, slot)) return rc;
  const ShardLayout l(q_per_owner, slot);
  try {
    HIP_OK(hipSetDevice(h->device));
    ensure_xbuf(b, l.total(W), W);
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return step_emit_into(h, b, W, l, b->x.send, 0);
}

// A deferred group's replays not yet enqueued go to the communicator's
// stream (after its all-to-all, which the worker has enqueued first).
static void flush_group(wsr_comm* c, XGroup& g) {
  while (!g.enq.load(std::memory_order_acquire)) std::this_thread::yield();
  int rc = c->err.load() == WSR_OK ? WSR_OK : WSR_E_HIP;
  for (size_t i = 0; i < g.bs.size(); ++i) {
    if (g.queued[i]) continue;
    g.queued[i] = 1;
    c->replays_stream.fetch_add(1);
    if (rc == WSR_OK && (rc = group_replay_on_stream(c, g, i))) set_comm_err(c, rc, g_err);
    g.bs[i]->x.enqueued(rc == WSR_OK, true);
  }
  c->xs[g.xs].n_done = g.bs.size();
}

// Enqueue the deferred replays of every pending group up to the one holding
// `upto` (all of them: upto null), oldest first.
static void replay_flush(wsr_comm* c, const wsr_batch* upto) {
  std::lock_guard<std::recursive_mutex> lk(c->pend_mu);
  if (upto) {
    bool held = false;
    for (const auto& g : c->pend)
      for (size_t i = 0; i < g->bs.size(); ++i) held = held || (!g->queued[i] && g->bs[i] == upto);
    if (!held) return;
  }
  while (!c->pend.empty()) {
    std::shared_ptr<XGroup> g = c->pend.front();
    c->pend.pop_front();
    bool has = false;
    for (size_t i = 0; i < g->bs.size(); ++i) has = has || (!g->queued[i] && g->bs[i] == upto);
    flush_group(c, *g);
    if (has) return;
  }
}

extern "C" {

int wsr_comm_flush(wsr_comm* c) {
  if (!c) return fail(WSR_E_INVALID, "null argument");
  try {
    HIP_OK(hipSetDevice(c->device));
    replay_flush(c, nullptr);
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  if (const int e = c->err.load()) {
    std::lock_guard<std::mutex> g(c->mu);
    return fail(e, "exchange: " + c->err_msg);
  }
  return WSR_OK;
}

int wsr_comm_stats_get(wsr_comm* c, wsr_comm_stats* out) {
  if (!c || !out) return fail(WSR_E_INVALID, "null argument");
  std::lock_guard<std::recursive_mutex> lk(c->pend_mu);
  out->groups = static_cast<int64_t>(c->n_groups);
  out->steps = static_cast<int64_t>(c->steps);
  out->replays_in_lean = c->replays_lean.load();
  out->replays_on_stream = c->replays_stream.load();
  return WSR_OK;
}

// A step group: n batches of the same shape, each emitted into its region of
// every owner's run of n regions in one of the communicator's exchange buffer
// sets, then ONE ncclAllToAll of the runs on the communicator's stream.  The
// collective's host cost (~0.1-0.2 ms a call under load, more than a whole
// step's kernels) is paid once per group.  The group's owner replays run on
// the communicator's stream too, or (deferred, the default) in the lean
// kernels of the group kReplayLag groups later: batch i of this group replays
// batch i of that one after its own items.
int wsr_shard_steps(wsr_handle* h, wsr_batch* const* bs, int32_t n, wsr_comm* c, int32_t q_per_owner,
                    int64_t slot) {
  if (!c || !bs || n < 1) return fail(WSR_E_INVALID, "bad shard_steps arguments");
  if (const int e = c->err.load()) {   // an earlier exchange of this communicator failed
    std::lock_guard<std::mutex> g(c->mu);
    return fail(e, "exchange worker: " + c->err_msg);
  }
  const int W = c->world;
  for (int i = 0; i < n; ++i) {
    if (int rc = check_step(h, bs[i], W, q_per_owner, slot)) return rc;
    for (int j = 0; j < i; ++j)
      if (bs[j] == bs[i]) return fail(WSR_E_INVALID, "a batch twice in one step group");
  }
  uint64_t t0 = c->timing ? now_ns() : 0;
  auto lap = [&](int i) {
    if (!c->timing) return;
    const uint64_t t = now_ns();
    c->t_ns[i] += t - t0;
    t0 = t;
  };
  std::lock_guard<std::recursive_mutex> pend_lock(c->pend_mu);
  const int xs = static_cast<int>(c->n_groups % kXSlots);
  XSlot& S = c->xs[xs];
  auto g = std::make_shared<XGroup>(h, bs, n, q_per_owner, slot, xs, c->defer);
  std::shared_ptr<XGroup> P;   // the group whose replays this one's lean kernels take
  // Once P is off pend, every exit enqueues what its lean kernels did not
  // take on the communicator's stream: on an early error return its batches
  // would otherwise wait in their join for replays nobody can find any more.
  struct FlushRest {
    wsr_comm* c;
    std::shared_ptr<XGroup>& P;
    ~FlushRest() {
      if (P) flush_group(c, *P);
    }
  } flush_rest{c, P};
  std::vector<OwnerJob> oj(static_cast<size_t>(n));
  try {
    HIP_OK(hipSetDevice(h->device));
    // this group's batches: their own earlier replays enqueued first
    for (int i = 0; i < n; ++i) {
      ensure_xev(bs[i]);
      if (bs[i]->x.comm.load(std::memory_order_acquire)) replay_flush(c, bs[i]);
    }
    // the slot: its previous group's all-to-all and replays enqueued (their
    // end events are what this group's emission and exchange wait for)
    if (S.last) {
      for (size_t i = 0; i < S.last->queued.size(); ++i)
        if (!S.last->queued[i]) replay_flush(c, S.last->bs[i]);
      while (!S.last->enq.load(std::memory_order_acquire)) std::this_thread::yield();
    }
    const uint64_t need = g->layout.total(static_cast<uint64_t>(W));
    if (need > S.send.size()) {
      if (S.last) {
        HIP_OK(hipEventSynchronize(S.xa));
        for (size_t i = 0; i < S.n_done; ++i) HIP_OK(hipEventSynchronize(S.done[i]));
        S.last.reset();
        S.n_done = 0;
      }
      gpu::alloc_group(need, S.send, S.recv);
    }
    if (!S.xa) S.xa = gpu::make_event();
    while (S.done.size() < static_cast<size_t>(n)) S.done.push_back(gpu::make_event());
    // the deferred replays this group's lean kernels take
    if (c->defer && c->pend.size() >= kReplayLag) {
      P = c->pend.front();
      c->pend.pop_front();
      while (!P->enq.load(std::memory_order_acquire)) std::this_thread::yield();
      for (size_t i = 0; i < P->bs.size() && i < static_cast<size_t>(n); ++i) {
        const wsr_batch* pb = P->bs[i];
        if (P->queued[i]) continue;
        if (pb->cls.has_wide) continue;   // (the LDS heap: on the communicator's stream)
        oj[i] = owner_job_of(pb, c->xs[P->xs].recv, P->layout, i, c->rank, W);
      }
    }
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  for (int i = 0; i < n; ++i) {
    wsr_batch* b = bs[i];
    const OwnerJob* job = oj[i].nq > 0 ? &oj[i] : nullptr;
    try {
      if (S.last) HIP_OK(hipStreamWaitEvent(b->st, S.xa, 0));   // the slot's last all-to-all read its send buffer
      if (job) HIP_OK(hipStreamWaitEvent(b->st, c->xs[P->xs].xa, 0));
    } catch (const std::exception& e) {
      return fail(WSR_E_HIP, e.what());
    }
    if (int rc = step_emit_into(h, b, W, g->layout, S.send, static_cast<uint64_t>(i), job)) return rc;
    if (hipEventRecord(b->x.ev[0], b->st) != hipSuccess) return fail(WSR_E_HIP, "hipEventRecord failed");
    if (job) {   // P's batch i went with b's lean kernel: its end is behind that, on b's stream
      wsr_batch* pb = P->bs[static_cast<size_t>(i)];
      if (!record_replay_end(pb, c->xs[P->xs].done[static_cast<size_t>(i)], b->st))
        return fail(WSR_E_HIP, "hipEventRecord failed");
      P->queued[static_cast<size_t>(i)] = 1;
      c->replays_lean.fetch_add(1);
      pb->x.enqueued(true, true);
    }
  }
  // the rest of P (more batches than this group, or wide ones): the
  // communicator's stream
  if (P) flush_group(c, *P);
  P.reset();
  lap(0);
  // the exchange half: the communicator's worker thread enqueues it
  if (S.last) g->wait_done.assign(S.done.begin(), S.done.begin() + static_cast<std::ptrdiff_t>(S.n_done));
  S.last = g;
  S.n_done = 0;
  ++c->n_groups;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = 0; i < n; ++i) {
      bs[i]->x.request();
      if (g->defer) bs[i]->x.comm.store(c, std::memory_order_release);
    }
    c->jobs.push_back(g);
  }
  if (g->defer) c->pend.push_back(g);
  c->cv.notify_one();
  lap(1);
  c->steps += static_cast<uint64_t>(n);
  return WSR_OK;
}

int wsr_shard_step(wsr_handle* h, wsr_batch* b, wsr_comm* c, int32_t q_per_owner, int64_t slot) {
  return wsr_shard_steps(h, &b, 1, c, q_per_owner, slot);
}

int wsr_shard_step_regions(int32_t q_per_owner, int64_t slot, uint64_t* region_bytes) {
  if (q_per_owner <= 0 || slot <= 0 || !region_bytes) return fail(WSR_E_INVALID, "bad arguments");
  *region_bytes = ShardLayout::bytes(ShardLayout(q_per_owner, slot).region());
  return WSR_OK;
}

static int shard_step_emit(wsr_handle* h, wsr_batch* b, int32_t world, int32_t q_per_owner, int64_t slot,
                           void* host_send, bool wait) {
  if (!host_send) return fail(WSR_E_INVALID, "null host buffer");
  const int rc = step_emit(h, b, world, q_per_owner, slot);
  if (rc) return rc;
  try {
    HIP_OK(hipMemcpyAsync(host_send, b->x.send, ShardLayout::bytes(b->x.layout().total(world)),
                          hipMemcpyDeviceToHost, b->st));
    if (wait) HIP_OK(hipStreamSynchronize(b->st));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return WSR_OK;
}

int wsr_shard_step_emit(wsr_handle* h, wsr_batch* b, int32_t world, int32_t q_per_owner, int64_t slot,
                        void* host_send) {
  return shard_step_emit(h, b, world, q_per_owner, slot, host_send, true);
}

int wsr_shard_step_emit_async(wsr_handle* h, wsr_batch* b, int32_t world, int32_t q_per_owner, int64_t slot,
                              void* host_send) {
  return shard_step_emit(h, b, world, q_per_owner, slot, host_send, false);
}

// The second half's arguments (the regions are read at the strides the
// emission wrote them with: they must be the ones of the preceding
// wsr_shard_step_emit), then the received regions' copy into b's buffer.
static int replay_regions_in(wsr_handle* h, wsr_batch* b, int32_t rank, int32_t world, int32_t q_per_owner,
                             int64_t slot, const void* host_recv) {
  if (!h || !b || !host_recv || world < 1 || rank < 0 || rank >= world || q_per_owner <= 0 || slot <= 0 ||
      !b->x.fused || b->x.world != world || b->x.qpr != q_per_owner || b->x.slot != slot ||
      static_cast<int64_t>(q_per_owner) * world != b->nq)
    return fail(WSR_E_INVALID, "call wsr_shard_step_emit with the same world, q_per_owner and slot first");
  if (b->cls.has_or) return fail(WSR_E_INVALID, "a doc-range shard step cannot run a disjunctive query");
  return WSR_OK;
}

int wsr_shard_step_replay(wsr_handle* h, wsr_batch* b, int32_t rank, int32_t world, int32_t q_per_owner,
                          int64_t slot, const void* host_recv) {
  if (int rc = replay_regions_in(h, b, rank, world, q_per_owner, slot, host_recv)) return rc;
  try {
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipMemcpyAsync(b->x.recv, host_recv, ShardLayout::bytes(b->x.layout().total(world)),
                          hipMemcpyHostToDevice, b->st));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  return own_replay_on(h, b, rank, b->st);
}

// Host-exchange owner replays deferred into a later run's lean kernel (the
// counterpart of the communicator's deferral, wsr_shard_steps): a separate
// owner replay launch -- thousands of one-wave workgroups -- costs more than
// its work beside the persistent kernels of the next batches.
int wsr_shard_step_replay_deferred(wsr_handle* h, wsr_batch* b, int32_t rank, int32_t world, int32_t q_per_owner,
                                   int64_t slot, const void* host_recv) {
  if (int rc = replay_regions_in(h, b, rank, world, q_per_owner, slot, host_recv)) return rc;
  if (b->cls.has_wide)   // (the LDS heap: the replay launch of its own)
    return wsr_shard_step_replay(h, b, rank, world, q_per_owner, slot, host_recv);
  try {
    HIP_OK(hipSetDevice(h->device));
    if (b->x.hdef) host_replay_flush(b);   // (an earlier one still waiting: first)
    ensure_xev(b);
    HIP_OK(hipMemcpyAsync(b->x.recv, host_recv, ShardLayout::bytes(b->x.layout().total(world)),
                          hipMemcpyHostToDevice, b->st));
    HIP_OK(hipEventRecord(b->x.ev[0], b->st));
  } catch (const std::exception& e) {
    return fail(WSR_E_HIP, e.what());
  }
  std::lock_guard<std::mutex> g(h->hdef_mu);
  b->x.hdef_rank = rank;
  b->x.hdef.store(h);
  h->hdef_q.push_back(b);
  return WSR_OK;
}

}  // extern "C"

wsr_batch* take_host_replay(wsr_handle* h, const wsr_batch* b, OwnerJob* oj) {
  std::lock_guard<std::mutex> g(h->hdef_mu);
  for (auto it = h->hdef_q.begin(); it != h->hdef_q.end(); ++it) {
    wsr_batch* pb = *it;
    if (pb == b) continue;
    h->hdef_q.erase(it);
    // counted before hdef is cleared: a join that sees it cleared waits
    // until the taking run has recorded x.ev[1] (enqueued)
    pb->x.request();
    pb->x.hdef.store(nullptr);
    *oj = owner_job_of(pb, pb->x.recv, pb->x.layout(), 0, pb->x.hdef_rank, pb->x.world);
    return pb;
  }
  return nullptr;
}

bool host_replay_enqueue(wsr_batch* pb, wsr_handle* h) {
  return own_replay_on(h, pb, pb->x.hdef_rank, pb->st) == WSR_OK &&
         hipEventRecord(pb->x.ev[1], pb->st) == hipSuccess;
}

// b's own deferred host replay, still queued: on its own stream now.
static void host_replay_flush(wsr_batch* b) {
  wsr_handle* h = b->x.hdef.load();
  if (!h) return;
  {
    std::lock_guard<std::mutex> g(h->hdef_mu);
    if (!b->x.hdef.load()) return;   // (taken by a run meanwhile; join waits for its enqueue)
    for (auto it = h->hdef_q.begin(); it != h->hdef_q.end(); ++it)
      if (*it == b) {
        h->hdef_q.erase(it);
        break;
      }
    b->x.request();   // (as take_host_replay)
    b->x.hdef.store(nullptr);
  }
  b->x.enqueued(host_replay_enqueue(b, h), false);
}
