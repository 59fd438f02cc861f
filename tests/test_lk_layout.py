"""lk_layout.h on the host: the lane -> window pixel ownership of lk_track_kernel covers the 21 x 21 window once, every window
read is free of LDS bank conflicts under the header's model (32 dword banks, lanes 0-31 and 32-63 served apart), and the model
gives the extra cycles of the PREVIOUS layout (lane l on column l % 21 of rows l / 21 + 3 q; strides 43 / 25 / 22) that the
kernel's bank-conflict counters were taken on: +2, +2, +1 per dword read."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "vins-mobile_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "lk_layout.h"
using namespace lk_layout;

// the previous ownership: lane l on column l % 21 of rows min(l / 21, 2) + 3 q
static int old_read(int stride, int q, int dy, int dx) {
  int addr[kLanes];
  for (int l = 0; l < kLanes; l++) {
    const int g = l / kWin < 2 ? l / kWin : 2;
    addr[l] = (g + 3 * q + dy) * stride + l % kWin + dx;
  }
  return lds_extra_cycles(addr);
}

static_assert(window_reads_extra_cycles(kStrideI) == 0 && window_reads_extra_cycles(kStrideDI) == 0 &&
                  window_reads_extra_cycles(kStrideJ) == 0, "usable in constant expressions");

int main() {
  // coverage: pixels (row + q, col) of lanes 0..62
  int seen[kWin][kWin] = {};
  int outside = 0;
  for (int l = 0; l < kOwners; l++)
    for (int q = 0; q < kPxPerLane; q++) {
      const Px p = lane_pixel0(l);
      const int r = p.row + q, c = p.col;
      if (r < 0 || r >= kWin || c < 0 || c >= kWin) outside++;
      else seen[r][c]++;
    }
  int once = 0;
  for (int r = 0; r < kWin; r++)
    for (int c = 0; c < kWin; c++) once += seen[r][c] == 1;
  printf("outside %d\n", outside);
  printf("once %d\n", once);
  // lane 63 owns nothing and reads what an owner reads
  const Px s = lane_pixel0(63);
  int shadows = 0;
  for (int l = 0; l < kOwners; l++) shadows += lane_pixel0(l).row == s.row && lane_pixel0(l).col == s.col;
  printf("shadows %d\n", shadows);
  // every window read: rows row0 + dy (dy 0..8: seven pixels, the row below, the patch's halo row), columns col0 + dx
  // (dx 0..2), at every base offset mod 32 (the J region's moving origin)
  const int strides[3] = {kStrideI, kStrideDI, kStrideJ};
  for (int a = 0; a < 3; a++) {
    int worst = 0;
    for (int dy = 0; dy <= kPxPerLane + 1; dy++)
      for (int dx = 0; dx <= 2; dx++)
        for (int base = 0; base < 2 * kBanks; base++) {
          const int e = window_read_extra_cycles(strides[a], dy, dx, base);
          worst = e > worst ? e : worst;
        }
    printf("new_%d %d\n", a, worst);
  }
  // the previous layout: J at 43 and at 29, I at 25, dI at 22; the same for every pixel and tap
  const int olds[4] = {43, 29, 25, 22};
  for (int a = 0; a < 4; a++) {
    int lo = 1 << 30, hi = 0;
    for (int q = 0; q < kPxPerLane; q++)
      for (int dy = 0; dy <= 2; dy++)
        for (int dx = 0; dx <= 1; dx++) {
          const int e = old_read(olds[a], q, dy, dx);
          lo = e < lo ? e : lo, hi = e > hi ? e : hi;
        }
    printf("old_%d_lo %d\nold_%d_hi %d\n", olds[a], lo, olds[a], hi);
  }
  // the model itself on patterns with known answers
  int addr[kLanes];
  for (int l = 0; l < kLanes; l++) addr[l] = l;
  printf("linear %d\n", lds_extra_cycles(addr));
  for (int l = 0; l < kLanes; l++) addr[l] = 7;
  printf("broadcast %d\n", lds_extra_cycles(addr));
  for (int l = 0; l < kLanes; l++) addr[l] = 2 * l;
  printf("stride2 %d\n", lds_extra_cycles(addr));
  for (int l = 0; l < kLanes; l++) addr[l] = 32 * l;
  printf("onebank %d\n", lds_extra_cycles(addr));
  for (int l = 0; l < kLanes; l++) addr[l] = l < 32 ? l : 32 * l;
  printf("halfbad %d\n", lds_extra_cycles(addr));
  printf("lds_bytes %d\n", 4 * ((24 * kStrideI + 22 * kStrideDI) > 28 * kStrideJ ? (24 * kStrideI + 22 * kStrideDI) : 28 * kStrideJ));
  return 0;
}
"""


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    d = tmp_path_factory.mktemp("lk_layout")
    src, exe = str(d / "lk_layout_check.cpp"), str(d / "lk_layout_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, src])
    out = subprocess.check_output([exe], text=True)
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_ownership_covers_the_window_once(figures):
    assert figures["outside"] == 0
    assert figures["once"] == 21 * 21  # 63 lanes x 7 pixels = 441 = every pixel exactly once
    assert figures["shadows"] == 1     # lane 63 repeats one owner's addresses: a broadcast, not a conflict


def test_window_reads_are_conflict_free(figures):
    assert figures["new_0"] == 0  # I
    assert figures["new_1"] == 0  # dI
    assert figures["new_2"] == 0  # J


def test_model_gives_the_previous_layouts_conflicts(figures):
    for stride, extra in ((43, 2), (29, 2), (25, 2), (22, 1)):
        assert figures["old_%d_lo" % stride] == extra and figures["old_%d_hi" % stride] == extra, stride


def test_model_on_known_patterns(figures):
    assert figures["linear"] == 0 and figures["broadcast"] == 0
    assert figures["stride2"] == 2    # 2-way in both lane groups
    assert figures["onebank"] == 62   # 32-way in both
    assert figures["halfbad"] == 31   # lanes 0-31 clean, lanes 32-63 32-way


def test_lds_fits_six_workgroups_per_cu(figures):
    assert figures["lds_bytes"] == 5336
    assert 4 * 6 * figures["lds_bytes"] <= 160 * 1024
