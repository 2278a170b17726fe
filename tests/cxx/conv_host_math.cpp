// Host check of tensor-fft_amd/conv/host_math.hpp, the arithmetic the nine convolution libraries share: the overlap test against
// brute force, the binary16 conversion round trip, the overlap-save geometry against the closed forms of tests/sconv_ref.py, and
// filter_slot as a permutation. Includes that header alone: it is plain C++17 and needs neither HIP nor a library.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../tensor-fft_amd/conv/host_math.hpp"

namespace hm = host_math;

// count blocks of len halves, stride halves apart, starting at half `first` of a range: one mark per half
static std::vector<int> marks(int64_t first, uint64_t stride, uint64_t len, uint64_t count, size_t range) {
  std::vector<int> m(range, 0);
  for (uint64_t i = 0; i < count; ++i)
    for (uint64_t j = 0; j < len; ++j) m[static_cast<size_t>(first + static_cast<int64_t>(i * stride + j))] = 1;
  return m;
}

static int check_seqs_overlap() {
  const uint64_t counts[] = {1, 2, 3}, strides[] = {8, 16, 24}, lens[] = {0, 8, 16};
  const int64_t origin = 128;                    // half index of base a: room for three strides of 24 below it
  const size_t range = 512;
  const uintptr_t range_base = 0x100000;         // addresses are compared, never dereferenced
  for (uint64_t count : counts)
    for (uint64_t sa : strides)
      for (uint64_t sb : strides)
        for (uint64_t la : lens)
          for (uint64_t lb : lens) {
            const std::vector<int> ma = marks(origin, sa, la, count, range);
            const int64_t reach = 3 * static_cast<int64_t>(sa > sb ? sa : sb);
            for (int64_t off = -reach; off <= reach; ++off) {
              const std::vector<int> mb = marks(origin + off, sb, lb, count, range);
              bool brute = false;
              for (size_t i = 0; i < range; ++i) brute = brute || (ma[i] && mb[i]);
              const void* pa = reinterpret_cast<const void*>(range_base + 2 * static_cast<uintptr_t>(origin));
              const void* pb = reinterpret_cast<const void*>(range_base + 2 * static_cast<uintptr_t>(origin + off));
              const bool got = hm::seqs_overlap(pa, sa, la, pb, sb, lb, count);
              if (brute && !got) {
                std::printf("seqs_overlap missed a shared half: count %llu sa %llu la %llu sb %llu lb %llu offset %lld\n",
                            (unsigned long long)count, (unsigned long long)sa, (unsigned long long)la, (unsigned long long)sb,
                            (unsigned long long)lb, (long long)off);
                return 1;
              }
              if (got && !brute && sa == sb) {
                std::printf("seqs_overlap is not exact at equal strides: count %llu stride %llu la %llu lb %llu offset %lld\n",
                            (unsigned long long)count, (unsigned long long)sa, (unsigned long long)la, (unsigned long long)lb, (long long)off);
                return 1;
              }
            }
          }
  return 0;
}

// The same test with blocks beyond 2^33 bytes of one allocation (tests/far_layout.py, layout `wide`): the interval arithmetic must
// neither wrap nor lose the high half of (count - 1) * stride. Addresses are compared, never dereferenced.
static int check_seqs_overlap_far() {
  const uint64_t stride = (uint64_t{1} << 31) + 8, count = 3, len = 4104;
  const uintptr_t base = uintptr_t{0x7f00} << 32;           // where a device allocation may lie
  auto at = [&](uint64_t half) { return reinterpret_cast<const void*>(base + 2 * static_cast<uintptr_t>(half)); };
  static_assert(sizeof(uintptr_t) == 8, "the far cases need 64-bit addresses");
  if (2 * (2 * stride) <= (uint64_t{1} << 33)) return 1;    // block 2 of either set starts beyond 2^33 bytes
  struct row {
    uint64_t a_first, sa, la, b_first, sb, lb;
    bool want;
    const char* what;
  };
  const row rows[] = {
      {0, stride, len, len + 16, stride, len, false, "interleaved sets whose blocks do not touch"},
      {0, stride, len, len, stride, len, false, "interleaved sets whose blocks abut"},
      {len + 16, stride, len, 0, stride, len, false, "interleaved sets, the other way round"},
      {0, stride, len, len - 1, stride, len, true, "the last half of every block of a is the first of b's, block 2 beyond 2^33 bytes"},
      {len - 1, stride, len, 0, stride, len, true, "the same, the other way round"},
      {0, stride, len, stride, stride, len, true, "b starts at a's block 1"},
      // b shifted by two strides: its blocks 1 and 2 lie beyond a's extent, its block 0 meets a's block 2 alone
      {0, stride, len, 2 * stride + len - 1, stride, len, true, "b's block 0 shares ONE half with a's block 2, beyond 2^33 bytes"},
      {0, stride, len, 2 * stride + len, stride, len, false, "b begins where a's block 2 ends"},
      {0, stride, len, 2 * stride + len - 1, stride + 16, len, true, "unequal strides, overlapping extents"},
      {0, stride, len, len + 16, stride + 16, len, true, "unequal strides, overlapping extents: conservative"},
      {0, stride, len, 2 * stride + len, stride + 16, len, false, "unequal strides, disjoint extents"},
  };
  for (const row& r : rows) {
    const bool got = hm::seqs_overlap(at(r.a_first), r.sa, r.la, at(r.b_first), r.sb, r.lb, count);
    if (got != r.want) {
      std::printf("seqs_overlap far: %s: got %d, want %d\n", r.what, int(got), int(r.want));
      return 1;
    }
  }
  return 0;
}

static int check_half_round_trip() {
  for (uint32_t h = 0; h < 65536; ++h) {
    const uint16_t back = hm::to_half(hm::from_half(static_cast<uint16_t>(h)));
    const bool is_nan = (h & 0x7c00) == 0x7c00 && (h & 0x03ff);
    const bool same = is_nan ? ((back & 0x7c00) == 0x7c00 && (back & 0x03ff)) : back == h;
    if (!same) {
      std::printf("to_half(from_half(0x%04x)) = 0x%04x\n", h, back);
      return 1;
    }
  }
  return 0;
}

static int check_geometry() {
  // halo = ceil((taps - 1) / 64) * 64, hop = 4096 - halo, segments = ceil(length / hop): tests/sconv_ref.py, geometry()
  struct row {
    uint64_t taps, halo, hop, segments_at_2_26;
  };
  const row rows[] = {{1, 0, 4096, 16384}, {2, 64, 4032, 16645}, {64, 64, 4032, 16645}, {65, 64, 4032, 16645}, {2049, 2048, 2048, 32768}};
  for (const row& r : rows) {
    if (hm::halo_of(r.taps) != r.halo || hm::hop_of(r.taps) != r.hop) {
      std::printf("taps %llu: halo %llu hop %llu\n", (unsigned long long)r.taps, (unsigned long long)hm::halo_of(r.taps),
                  (unsigned long long)hm::hop_of(r.taps));
      return 1;
    }
    const uint64_t lengths[] = {8, r.hop, r.hop + 8, uint64_t{1} << 26}, want[] = {1, 1, 2, r.segments_at_2_26};
    for (int i = 0; i < 4; ++i)
      if (hm::segments_of(lengths[i], r.taps) != want[i]) {
        std::printf("taps %llu length %llu: %llu segments, not %llu\n", (unsigned long long)r.taps, (unsigned long long)lengths[i],
                    (unsigned long long)hm::segments_of(lengths[i], r.taps), (unsigned long long)want[i]);
        return 1;
      }
  }
  return 0;
}

static int check_filter_slot() {
  static_assert(hm::filter_slot(0) == 0, "filter_slot is a constant expression");
  std::vector<int> seen(4096, 0);
  for (uint32_t k = 0; k < 4096; ++k) {
    const uint32_t slot = hm::filter_slot(k);
    if (slot >= 4096 || seen[slot]++) {
      std::printf("filter_slot(%u) = %u is out of range or taken\n", k, slot);
      return 1;
    }
  }
  return 0;
}

int main() {
  if (check_seqs_overlap() || check_seqs_overlap_far() || check_half_round_trip() || check_geometry() || check_filter_slot()) return 1;
  std::printf("ok\n");
  return 0;
}
