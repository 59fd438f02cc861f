// lk_track_kernel's 21 x 21 window in LDS: which lane owns which window pixel, the row strides of the staged arrays, and a
// model of the LDS bank conflicts of a wave64 dword read. Plain C++ (no HIP): the kernel static_asserts on the model, and
// tests/test_lk_layout.py compiles it for the host.
//
// The banking rule (ds_read_b32, and each half of a ds_read2_b32): a wave64 read is served in two lane groups, lanes 0-31 and
// lanes 32-63; the bank of a dword is (byte address / 4) mod 32; lanes of a group that read the same dword share one access
// (broadcast); every further distinct dword on a bank that is already busy in the group costs one more LDS-array cycle, so a
// group takes as many cycles as its busiest bank holds distinct dwords.
#pragma once

namespace lk_layout {

constexpr int kWin = 21;            // window side
constexpr int kLanes = 64;          // wave size
constexpr int kBanks = 32;          // dword banks seen by a 4-byte read
constexpr int kBankGroup = 32;      // lanes served together
constexpr int kPxPerLane = 7;       // (21 * 21 + 63) / 64
constexpr int kOwners = 3 * kWin;   // lanes 0..62 own pixels; lane 63 owns none

// Row stride in dwords of the staged template patch I, of its derivative image dI and of the staged J region. One value serves
// all three: with the ownership below the three lane groups start 7 rows apart, 7 * 29 = 11 and 14 * 29 = 22 (mod 32), and the
// middle group's rotation by 10 columns puts lanes 21-31 on banks 21..31 beside lanes 0-20 on banks 0..20, and lanes 32-41 on
// banks 11..20 beside lanes 42-62 on banks 22..31, 0..10. A shift of the whole pattern (the [y][x+1] and [y+1][.] taps, the J
// region's moving base) rotates every bank alike, so it stays conflict-free.
constexpr int kStrideI = 29, kStrideDI = 29, kStrideJ = 29;

struct Px {
  int row, col;
};
// First window pixel of a lane; its q-th pixel (q = 0..6) is (row + q, col): seven consecutive rows of one column, so the
// bottom row word of pixel q is the top row word of pixel q + 1. Lanes 0-20, 21-41, 42-62 own rows 0-6, 7-13, 14-20; the
// middle group's columns are rotated by 10. Lane 63 shadows lane 42's addresses (identical addresses broadcast).
constexpr Px lane_pixel0(int lane) {
  const int g = lane / kWin < 2 ? lane / kWin : 2;
  const int c = lane % kWin;
  return Px{kPxPerLane * g, g == 1 ? (c + 10) % kWin : c};
}

// Extra LDS-array cycles (beyond the two of a conflict-free read) of one wave64 dword read; addr[l] = dword address of lane l.
constexpr int lds_extra_cycles(const int (&addr)[kLanes]) {
  int extra = 0;
  for (int g0 = 0; g0 < kLanes; g0 += kBankGroup) {
    int cnt[kBanks] = {};
    for (int i = g0; i < g0 + kBankGroup; i++) {
      bool dup = false;
      for (int j = g0; j < i; j++) dup = dup || addr[j] == addr[i];
      if (!dup) cnt[((addr[i] % kBanks) + kBanks) % kBanks]++;
    }
    int worst = 1;
    for (int b = 0; b < kBanks; b++) worst = cnt[b] > worst ? cnt[b] : worst;
    extra += worst - 1;
  }
  return extra;
}

// The read of array element [row0 + dy][col0 + dx] by every lane, at `stride` dwords per row and `base` dwords in front.
constexpr int window_read_extra_cycles(int stride, int dy, int dx, int base = 0) {
  int addr[kLanes] = {};
  for (int l = 0; l < kLanes; l++) {
    const Px p = lane_pixel0(l);
    addr[l] = base + (p.row + dy) * stride + p.col + dx;
  }
  return lds_extra_cycles(addr);
}
// All window reads of a template build or an iteration: rows row0 .. row0 + 7 (+ 1 for the patch's halo), columns col0 .. col0 + 2.
constexpr int window_reads_extra_cycles(int stride) {
  int extra = 0;
  for (int dy = 0; dy <= kPxPerLane + 1; dy++)
    for (int dx = 0; dx <= 2; dx++) extra += window_read_extra_cycles(stride, dy, dx);
  return extra;
}

}  // namespace lk_layout
