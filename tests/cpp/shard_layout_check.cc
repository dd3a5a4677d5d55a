// CPU check of the shard exchange's region layout in wiser_amd/csrc/shard_layout.h
// (tests/test_shard_layout.py): the sizes against the formula written out here,
// every meta pair and slot inside the buffer and apart from the others, and
// the sender's view (emit_view_of) against the owner's (owner_job_of) through
// an all-to-all done here on arrays the test owns -- for a batch's own
// buffers (one batch) and a step group's (several).
// One "ok <case>" line per case; exit status 0.
#include "../../wiser_amd/csrc/shard_layout.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace wiser;

namespace {

#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      std::fprintf(stderr, "shard_layout_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                       \
    }                                                                                     \
  } while (0)

void ok(const char* name) { std::printf("ok %s\n", name); }

const int kWorlds[] = {1, 2, 3, 8};
const int32_t kQprs[] = {1, 2, 3, 8};
const int64_t kSlots[] = {1, 5};
const uint64_t kBatches[] = {1, 3};
constexpr uint64_t kWordsPerEvent = 4;   // int32 in a 16-byte event

template <class F>
void for_each_shape(F f) {
  for (int W : kWorlds)
    for (int32_t qpr : kQprs)
      for (int64_t slot : kSlots)
        for (uint64_t n : kBatches) f(W, qpr, slot, n);
}

// the sender's addresses, as FusedReplay::meta_of and the emission (kernels.h) form them
int32_t* emit_meta(const EmitView& v, int o, int32_t q) { return v.meta + o * v.meta_stride + 2ull * q; }
Event* emit_slot(const EmitView& v, int o) { return v.send + o * v.stride; }
// the owner's, as owner_replay_query (kernels.hip) forms them
const int32_t* owner_meta(const OwnerJob& j, int g, int32_t q) { return j.meta + g * j.meta_stride + 2ull * q; }
const Event* owner_slot(const OwnerJob& j, int g) { return j.recv + g * j.stride; }

void sizes_case() {
  static_assert(sizeof(Event) == 4 * sizeof(int32_t), "an event holds two meta pairs");
  for_each_shape([](int W, int32_t qpr, int64_t slot, uint64_t n) {
    const ShardLayout l(qpr, slot, n);
    const uint64_t region = (static_cast<uint64_t>(qpr) + 1) / 2 + static_cast<uint64_t>(slot);
    CHECK(l.meta_events() == (static_cast<uint64_t>(qpr) + 1) / 2);
    CHECK(l.region() == region);
    CHECK(l.run() == region * n);
    CHECK(l.total(W) == region * n * W);
    CHECK(l.meta_stride() == region * n * kWordsPerEvent);
    CHECK(l.slot_at() == l.meta_events());
    for (uint64_t i = 0; i < n; ++i) CHECK(l.batch_at(i) == region * i);
    // wsr_shard_step_regions' answer: the bytes of one region of a single batch
    CHECK(ShardLayout::bytes(ShardLayout(qpr, slot).region()) == 16 * region);
    CHECK(ShardLayout::bytes(l.total(W)) == 16 * region * n * W);
  });
  static_assert(ShardLayout(3, 5, 2).run() == 14, "constexpr");
  ok("sizes");
}

// Every (owner, batch, query) meta pair and every (owner, batch) slot of a
// send buffer inside it, no int32 of it claimed twice; a region's meta block
// ends where its slot begins.  The same for what an owner reads of its
// receive buffer.
void ranges_case() {
  for_each_shape([](int W, int32_t qpr, int64_t slot, uint64_t n) {
    const ShardLayout l(qpr, slot, n);
    std::vector<Event> buf(l.total(W));
    const int32_t* w0 = reinterpret_cast<const int32_t*>(buf.data());
    const uint64_t words = l.total(W) * kWordsPerEvent;
    for (int side = 0; side < 2; ++side) {   // 0: a sender's buffer, 1: an owner's (rank 0's)
      std::vector<uint8_t> used(words, 0);
      auto claim = [&](const void* p, uint64_t n_words) {
        const int32_t* w = static_cast<const int32_t*>(p);
        CHECK(w >= w0 && static_cast<uint64_t>(w - w0) + n_words <= words);
        for (uint64_t k = 0; k < n_words; ++k) {
          CHECK(!used[(w - w0) + k]);
          used[(w - w0) + k] = 1;
        }
      };
      for (uint64_t i = 0; i < n; ++i) {
        const EmitView v = emit_view_of(buf.data(), l, i, W);
        const OwnerJob j = owner_job_of(OwnerJob{}, buf.data(), l, i, 0, W);
        CHECK(v.owners == W && v.qpr == qpr && v.slot == static_cast<uint64_t>(slot));
        CHECK(j.q0 == 0 && j.nq == qpr && j.n_shards == W);
        for (int o = 0; o < W; ++o) {   // (the owner of a sender's run; the shard of an owner's)
          const int32_t* m0 = side ? owner_meta(j, o, 0) : emit_meta(v, o, 0);
          const Event* s0 = side ? owner_slot(j, o) : emit_slot(v, o);
          for (int32_t q = 0; q < qpr; ++q) claim(side ? owner_meta(j, o, q) : emit_meta(v, o, q), 2);
          claim(s0, static_cast<uint64_t>(slot) * kWordsPerEvent);
          CHECK(reinterpret_cast<const Event*>(m0) + l.meta_events() == s0);
        }
      }
      // all but the padding of an odd qpr's last meta event is claimed
      uint64_t n_used = 0;
      for (uint8_t u : used) n_used += u;
      CHECK(n_used == words - (qpr % 2) * 2ull * n * W);
    }
  });
  ok("ranges");
}

// Sender and owner agree.  Every sender g writes, through its emission views,
// a code of (g, owner, batch, query) into the query's pair and a code of (g,
// owner, batch, event) into every event of the slot; the all-to-all moves
// sender g's run for owner o to run g of owner o's receive buffer; the
// OwnerJob of rank o then reads exactly the codes written for it, and at the
// same place of the run.
void agree_case() {
  for_each_shape([](int W, int32_t qpr, int64_t slot, uint64_t n) {
    const ShardLayout l(qpr, slot, n);
    auto code = [&](int g, int o, uint64_t i, int64_t k) {
      return static_cast<int32_t>(((g * W + o) * static_cast<int64_t>(n) + static_cast<int64_t>(i)) * 64 + k + 1);
    };
    std::vector<std::vector<Event>> send(W, std::vector<Event>(l.total(W))), recv = send;
    for (int g = 0; g < W; ++g)
      for (uint64_t i = 0; i < n; ++i) {
        const EmitView v = emit_view_of(send[g].data(), l, i, W);
        for (int o = 0; o < W; ++o) {
          for (int32_t q = 0; q < qpr; ++q) {
            emit_meta(v, o, q)[0] = code(g, o, i, q);
            emit_meta(v, o, q)[1] = -code(g, o, i, q);
          }
          for (int64_t k = 0; k < slot; ++k) emit_slot(v, o)[k].doc = code(g, o, i, 8 + k);
        }
      }
    for (int g = 0; g < W; ++g)   // the all-to-all
      for (int o = 0; o < W; ++o)
        for (uint64_t e = 0; e < l.run(); ++e) recv[o][g * l.run() + e] = send[g][o * l.run() + e];
    for (int o = 0; o < W; ++o)
      for (uint64_t i = 0; i < n; ++i) {
        OwnerJob of{};
        of.hit_stride = 7;   // (the batch's part is kept)
        const OwnerJob j = owner_job_of(of, recv[o].data(), l, i, o, W);
        CHECK(j.hit_stride == 7 && j.q0 == o * qpr && j.nq == qpr && j.n_shards == W);
        for (int g = 0; g < W; ++g) {
          const EmitView v = emit_view_of(send[g].data(), l, i, W);
          const Event* sent_run = send[g].data() + o * l.run();
          const Event* got_run = recv[o].data() + g * l.run();
          for (int32_t q = 0; q < qpr; ++q) {
            CHECK(owner_meta(j, g, q)[0] == code(g, o, i, q) && owner_meta(j, g, q)[1] == -code(g, o, i, q));
            CHECK(owner_meta(j, g, q) - reinterpret_cast<const int32_t*>(got_run) ==
                  emit_meta(v, o, q) - reinterpret_cast<const int32_t*>(sent_run));
          }
          for (int64_t k = 0; k < slot; ++k) CHECK(owner_slot(j, g)[k].doc == code(g, o, i, 8 + k));
          CHECK(owner_slot(j, g) - got_run == emit_slot(v, o) - sent_run);
        }
      }
  });
  ok("sender_owner_agree");
}

// 64-bit arithmetic: a slot of 2^32 - 1 events and 1,024 queries per owner
void wide_case() {
  const uint64_t region = 512ull + 0xFFFFFFFFull;   // (1024 + 1) / 2 + slot
  static_assert(512ull + 0xFFFFFFFFull == 4294967807ull, "over 2^32");
  const ShardLayout l(1024, 0xFFFFFFFFll, 3);
  CHECK(l.meta_events() == 512 && l.slot_at() == 512);
  CHECK(l.region() == region);
  CHECK(l.run() == 3 * region);
  CHECK(l.total(8) == 24 * region);
  CHECK(l.batch_at(2) == 2 * region);
  CHECK(l.meta_stride() == 12 * region);
  CHECK(ShardLayout::bytes(ShardLayout(1024, 0xFFFFFFFFll).region()) == 16 * region);
  CHECK(ShardLayout::bytes(l.total(8)) == 384 * region);
  // the views' strides (batch 0: the addresses stay in the test's array)
  std::vector<Event> buf(513);
  const EmitView v = emit_view_of(buf.data(), l, 0, 8);
  CHECK(v.slot == 0xFFFFFFFFull && v.stride == 3 * region && v.meta_stride == 12 * region);
  CHECK(v.send == buf.data() + 512 && v.meta == reinterpret_cast<int32_t*>(buf.data()));
  const OwnerJob j = owner_job_of(OwnerJob{}, buf.data(), l, 0, 7, 8);
  CHECK(j.stride == 3 * region && j.meta_stride == 12 * region && j.q0 == 7 * 1024);
  CHECK(j.recv == buf.data() + 512 && j.meta == reinterpret_cast<const int32_t*>(buf.data()));
  ok("wide_arithmetic");
}

}  // namespace

int main() {
  sizes_case();
  ranges_case();
  agree_case();
  wide_case();
  return 0;
}
