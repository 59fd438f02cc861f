// valid_region_main.cpp — the valid region of a pre-step slot (csrc/pre_source.h, the text valid_region_kernel and
// vio_lens_model_valid_region compile) on the host, as a program of its own: tests/test_region_cpu.py builds it with
// -fsanitize=address,undefined, runs it and compares what it prints with the library's bytes. Built with -ffp-contract=off.
//   valid_region IN
//     IN : records, one per case: int32 rows, cols, margin, has_source; VioLensModel; VioSource (9 int32; when has_source)
//     prints one line per record: the CRC-32 of the mask's rows * cols bytes (zlib's polynomial) and the number of zeros
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pre_source.h"

static uint32_t crc32_of(const uint8_t *p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[4];
  while (fread(hdr, sizeof hdr, 1, f) == 1) {
    VioLensModel M;
    VioSource S;
    const int rows = hdr[0], cols = hdr[1], margin = hdr[2], has_source = hdr[3];
    if (fread(&M, sizeof M, 1, f) != 1 || (has_source && fread(&S, sizeof S, 1, f) != 1)) return 4;
    if (rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || margin < 0 || margin > pre::kRegionMaxMargin ||
        !pre::lens_model_valid(M) || (has_source && !pre::source_valid(S, rows, cols)))
      return 5;
    pre::SourcePlan plan;
    if (has_source) plan = pre::source_plan(S, rows, cols);
    std::vector<uint8_t> mask((size_t)rows * cols), tmp((size_t)rows * cols);
    pre::valid_region(&M, has_source ? &plan : nullptr, rows, cols, margin, mask.data(), tmp.data());
    size_t zeros = 0;
    for (uint8_t v : mask) zeros += v == 0;
    printf("%u %zu\n", crc32_of(mask.data(), mask.size()), zeros);
  }
  fclose(f);
  return 0;
}
