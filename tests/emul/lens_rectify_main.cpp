// lens_rectify_main.cpp — the per-pixel lens rectification of the image pre-step (csrc/pre_rectify.h, the text the device
// kernel compiles) on the host, as a program of its own: tests/test_lens_cpu.py compares its output with the numpy
// restatement of the arithmetic in include/vio_amd.h, bit for bit. Built with g++ -ffp-contract=off.
//   lens_rectify IN OUT
//   IN : int32 rows, cols, channels (1 | 4), 0; VioLens (13 doubles); rows * cols * channels bytes (packed rows)
//   OUT: rows * cols bytes, the rectified gray
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pre_rectify.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[4];
  VioLens L;
  if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(&L, sizeof L, 1, f) != 1) return 4;
  const int rows = hdr[0], cols = hdr[1], ch = hdr[2];
  if (rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || !(ch == 1 || ch == 4) || !pre::lens_valid(L)) return 5;
  std::vector<uint32_t> words(((size_t)rows * cols * ch + 3) / 4);  // 4-byte aligned, as the RGBA read wants it
  uint8_t *img = reinterpret_cast<uint8_t *>(words.data());
  if (fread(img, (size_t)rows * cols * ch, 1, f) != 1) return 6;
  fclose(f);
  std::vector<uint8_t> out((size_t)rows * cols);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++)
      out[(size_t)y * cols + x] = (uint8_t)(ch == 4 ? pre::rectify_px<4>(img, (size_t)cols * 4, rows, cols, L, x, y)
                                                    : pre::rectify_px<1>(img, (size_t)cols, rows, cols, L, x, y));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), out.size(), 1, f) != 1 || fclose(f) != 0) return 7;
  return 0;
}
