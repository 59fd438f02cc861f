// source_scale_main.cpp — the per-pixel arithmetic of a native-size source frame (csrc/pre_source.h, the text the device kernel
// compiles) on the host, as a program of its own: tests/test_source_cpu.py compares its output with the numpy restatement of
// include/vio_amd.h (tests/source_cases.py), bit for bit. Built with g++ -ffp-contract=off.
//   source_scale IN OUT
//   IN : int32 rows, cols (the output), has_lens, 0; VioSource (9 int32); VioLens (13 doubles; read when has_lens);
//        source.rows * source.stride bytes (plane 0 as delivered)
//   OUT: rows * cols bytes, the gray image of the slot
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pre_source.h"

template <int BPP, bool VIDEO>
static void run(const uint8_t *img, const pre::SourcePlan &P, const VioLens *L, int rows, int cols, uint8_t *out) {
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++)
      out[(size_t)y * cols + x] =
          (uint8_t)(L ? pre::rectify_source_px<BPP, VIDEO>(img, P, *L, x, y) : pre::area_px<BPP, VIDEO>(img, P, x, y));
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[4];
  VioSource S;
  VioLens L;
  if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(&S, sizeof S, 1, f) != 1 || fread(&L, sizeof L, 1, f) != 1) return 4;
  const int rows = hdr[0], cols = hdr[1], has_lens = hdr[2];
  if (!pre::source_valid(S, rows, cols) || (has_lens && !pre::lens_valid(L))) return 5;
  const size_t bytes = (size_t)S.rows * S.stride;
  std::vector<uint32_t> words((bytes + 3) / 4);  // 4-byte aligned, as the RGBA / BGRA read wants it
  uint8_t *img = reinterpret_cast<uint8_t *>(words.data());
  if (fread(img, bytes, 1, f) != 1) return 6;
  fclose(f);
  const pre::SourcePlan P = pre::source_plan(S, rows, cols);
  std::vector<uint8_t> out((size_t)rows * cols);
  const VioLens *lens = has_lens ? &L : nullptr;
  if (P.bpp == 4)
    run<4, false>(img, P, lens, rows, cols, out.data());
  else if (P.video)
    run<1, true>(img, P, lens, rows, cols, out.data());
  else
    run<1, false>(img, P, lens, rows, cols, out.data());
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), out.size(), 1, f) != 1 || fclose(f) != 0) return 7;
  return 0;
}
