// The region layout of the doc-range shard exchange, stated once for the
// sender (a batch run's fused emission), the transport (one all-to-all of
// equal runs) and the owner (the replay).  No HIP, no handle: the CPU check in
// tests/cpp/shard_layout_check.cc proves that the two device views below
// address the same events.  wiser_amd/shard.py::region_events restates the
// region size for the host exchange.
//
// A buffer holds, per owner, a run of n_batches regions (a step group's
// batches; 1: a batch's own buffers).  A region is the {count, offset} int32
// pairs of the owner's qpr queries, padded to whole events (4 int32 each),
// then the owner's slot of events.  The all-to-all moves sender g's run for
// owner o to run g of owner o's receive buffer.
#pragma once

#include <cstdint>

#include "engine_types.h"

namespace wiser {

struct ShardLayout {
  int32_t qpr;          // queries per owner
  uint64_t slot;        // capacity of an owner's slot (events)
  uint64_t n_batches;
  constexpr ShardLayout(int32_t q_per_owner, int64_t slot_events, uint64_t batches = 1)
      : qpr(q_per_owner), slot(static_cast<uint64_t>(slot_events)), n_batches(batches) {}
  // in events
  constexpr uint64_t meta_events() const { return (static_cast<uint64_t>(qpr) + 1) / 2; }
  constexpr uint64_t region() const { return meta_events() + slot; }
  constexpr uint64_t run() const { return region() * n_batches; }   // between owners
  constexpr uint64_t total(uint64_t world) const { return run() * world; }
  constexpr uint64_t batch_at(uint64_t i) const { return region() * i; }   // batch i's region in a run
  constexpr uint64_t slot_at() const { return meta_events(); }             // the slot in a region
  // in int32: between the owners' meta blocks
  constexpr uint64_t meta_stride() const { return run() * (sizeof(Event) / sizeof(int32_t)); }
  static constexpr uint64_t bytes(uint64_t events) { return events * sizeof(Event); }
};

// What batch `index` of the layout emits into, in the send buffer at base:
// FusedReplay::x_* (kernels.h) carries exactly this.  Query i of owner o has
// its pair at meta + o * meta_stride + 2 * i, owner o its slot at send + o *
// stride.
struct EmitView {
  int32_t owners;
  int32_t qpr;
  uint64_t slot;
  Event* send;
  uint64_t stride;
  int32_t* meta;
  uint64_t meta_stride;
};
inline EmitView emit_view_of(Event* base, const ShardLayout& l, uint64_t index, int32_t world) {
  Event* region = base + l.batch_at(index);
  return EmitView{world, l.qpr, l.slot, region + l.slot_at(), l.run(), reinterpret_cast<int32_t*>(region),
                  l.meta_stride()};
}

// The owner replay of batch `index` by `rank`, over the receive buffer at
// base.  of_batch: the replayed batch's own part (qs, hits, n_hits, counters,
// hit_stride).
inline OwnerJob owner_job_of(OwnerJob of_batch, const Event* base, const ShardLayout& l, uint64_t index,
                             int32_t rank, int32_t world) {
  const Event* region = base + l.batch_at(index);
  of_batch.meta = reinterpret_cast<const int32_t*>(region);
  of_batch.recv = region + l.slot_at();
  of_batch.meta_stride = l.meta_stride();
  of_batch.stride = l.run();
  of_batch.q0 = rank * l.qpr;
  of_batch.nq = l.qpr;
  of_batch.n_shards = world;
  return of_batch;
}

}  // namespace wiser
