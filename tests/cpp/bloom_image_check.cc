// CPU check of the bloom filters of a doc-range shard image
// (wiser_amd/csrc/index.cc, build_image's with_blm block): the filters of a
// list's bloom box b belong to the image's row b - r0 of that list, r0 = the
// list's first skip row in the image.  Builds the whole image and the image
// of every given doc range, with positions and blooms, and requires for every
// list and every block of a shard image, against the whole image's block of
// the same list with the same last doc id:
//   * the block's 128 x 32 filter bytes are equal;
//   * the slots past the box's postings are zero;
//   * blm_hash of the list, blm_bits and blm_hashes are equal.
// blank <term> <b,b,...> names the boxes (>= 0) whose filters the index lost
// (tests/bloom_tamper.py): in the whole image exactly those blocks of the term
// hold no set bit.  At least one compared block must be a blanked one and one
// not, and one shard image must start a list of several blocks past its first.
// Usage: bloom_image_check <vacuum_dir> [range <lo> <hi>]... [blank <term> <b,b,...>]...
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../wiser_amd/csrc/index.h"

using wiser::HostImage;
using wiser::ListDev;

constexpr uint64_t kSlots = 128, kSlotBytes = 32, kBlockBytes = kSlots * kSlotBytes;

static bool all_zero(const uint8_t* p, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (p[i]) return false;
  return true;
}

static int fail(const char* what, const std::string& term, uint64_t a, uint64_t b) {
  std::fprintf(stderr, "bloom_image_check: %s: list '%s' (%llu, %llu)\n", what, term.c_str(),
               static_cast<unsigned long long>(a), static_cast<unsigned long long>(b));
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <vacuum_dir> [range <lo> <hi>]... [blank <term> <b,b,...>]...\n", argv[0]);
    return 2;
  }
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  std::map<std::string, std::set<uint64_t>> blank;
  for (int i = 2; i < argc;) {
    if (!std::strcmp(argv[i], "range") && i + 2 < argc) {
      ranges.emplace_back(std::strtoul(argv[i + 1], nullptr, 10), std::strtoul(argv[i + 2], nullptr, 10));
    } else if (!std::strcmp(argv[i], "blank") && i + 2 < argc) {
      for (const char* p = argv[i + 2]; *p;) {
        char* e;
        blank[argv[i + 1]].insert(std::strtoull(p, &e, 10));
        p = *e ? e + 1 : e;
      }
    } else {
      std::fprintf(stderr, "bad argument '%s'\n", argv[i]);
      return 2;
    }
    i += 3;
  }
  wiser::VacuumIndex idx;
  idx.open(argv[1]);
  const HostImage whole = wiser::build_image(idx, 0, 0xFFFFFFFFu, 4, 0, true, 0, true);   // (wsr_open's whole range)
  if (!whole.has_blooms || whole.blm.size() != whole.blk_last.size() * kBlockBytes ||
      whole.blm_hash.size() != 2 * whole.lists.size()) {
    std::fprintf(stderr, "bloom_image_check: the whole image holds no filters\n");
    return 1;
  }
  // the whole image: every list's block r is its box r; slots past the box are zero, and the
  // blanked boxes, no others of their lists, hold no set bit
  for (int32_t id = 0; id < idx.n_lists(); ++id) {
    const ListDev& L = whole.lists[id];
    if (L.nblk != (L.df + kSlots - 1) / kSlots) return fail("whole image block count", idx.term(id), L.nblk, L.df);
    const auto bl = blank.find(idx.term(id));
    for (uint32_t r = 0; r < L.nblk; ++r) {
      const uint64_t n = std::min<uint64_t>(kSlots, L.df - kSlots * r);
      const uint8_t* p = &whole.blm[(L.blk0 + r) * kBlockBytes];
      if (!all_zero(p + n * kSlotBytes, (kSlots - n) * kSlotBytes)) return fail("set bits past the box", idx.term(id), r, n);
      if (bl != blank.end() && all_zero(p, kBlockBytes) != (bl->second.count(r) > 0))
        return fail("blanked boxes of the whole image", idx.term(id), r, bl->second.count(r));
    }
  }
  for (const auto& b : blank)
    if (idx.find(b.first) < 0) return fail("blank: no such term", b.first, 0, 0);
  uint64_t compared = 0, blanked = 0, filled = 0, late_starts = 0;
  for (const auto& rg : ranges) {
    const HostImage img = wiser::build_image(idx, rg.first, rg.second, 4, 0, true, 0, true);
    if (!img.has_blooms || img.blm_bits != whole.blm_bits || img.blm_hashes != whole.blm_hashes ||
        img.blm_hash != whole.blm_hash || img.blm.size() != img.blk_last.size() * kBlockBytes) {
      std::fprintf(stderr, "bloom_image_check: shard [%u, %u): filter shape or term hashes differ\n", rg.first,
                   rg.second);
      return 1;
    }
    for (int32_t id = 0; id < idx.n_lists(); ++id) {
      const ListDev& S = img.lists[id];
      const ListDev& L = whole.lists[id];
      const auto bl = blank.find(idx.term(id));
      for (uint32_t j = 0; j < S.nblk; ++j) {
        uint32_t r = 0;
        while (r < L.nblk && whole.blk_last[L.blk0 + r] != img.blk_last[S.blk0 + j]) ++r;
        if (r == L.nblk) return fail("no block of the whole image ends with this doc", idx.term(id), j, img.blk_last[S.blk0 + j]);
        if (j == 0 && r > 0 && L.nblk > 1) ++late_starts;
        const uint64_t n = std::min<uint64_t>(kSlots, L.df - kSlots * r);
        const uint8_t* s = &img.blm[(S.blk0 + j) * kBlockBytes];
        const uint8_t* w = &whole.blm[(L.blk0 + r) * kBlockBytes];
        if (std::memcmp(s, w, kBlockBytes)) return fail("filters differ from the whole image's (shard block, box)", idx.term(id), j, r);
        if (!all_zero(s + n * kSlotBytes, (kSlots - n) * kSlotBytes)) return fail("set bits past the box", idx.term(id), j, n);
        ++compared;
        if (bl != blank.end() && bl->second.count(r)) ++blanked;   // (all zero: checked on the whole image)
        else if (!all_zero(w, kBlockBytes)) ++filled;
      }
    }
  }
  std::printf("ranges %zu compared %llu blanked %llu filled %llu late_starts %llu\n", ranges.size(),
              static_cast<unsigned long long>(compared), static_cast<unsigned long long>(blanked),
              static_cast<unsigned long long>(filled), static_cast<unsigned long long>(late_starts));
  if (!blanked || !filled || !late_starts) {
    std::fprintf(stderr, "bloom_image_check: vacuous: no blanked block, no filled block or no shard starting past a "
                         "list's first box\n");
    return 1;
  }
  return 0;
}
