// lens_model_main.cpp — the lens models of the image pre-step (csrc/pre_rectify.h and pre_source.h, the text the device kernels
// compile) on the host, as a program of its own: tests/test_lens_models_cpu.py compares its output with the numpy restatement
// of the arithmetic (tests/lens_model_cases.py), bit for bit. Built with g++ -ffp-contract=off.
//   lens_model rectify IN OUT
//     IN : int32 rows, cols (the output), channels (1 | 4; not read with a source), has_source; VioLensModel;
//          VioSource (9 int32; read when has_source); the frame: rows * cols * channels bytes (packed rows), or with a source
//          source.rows * source.stride bytes (plane 0 as delivered)
//     OUT: rows * cols bytes, the rectified gray
//   lens_model atan IN OUT
//     IN : doubles x >= 0;  OUT: pre::lens_atan of each
//   lens_model layout
//     prints sizeof(VioLensModel) and the offsets of fx, k and rect_fx
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pre_source.h"

// the kernels' dispatch: the model is chosen once per frame, the pixel function is compiled for it
template <int MODEL>
static void rectify(const uint8_t *img, int ch, int rows, int cols, const VioLensModel &M, const pre::SourcePlan *P, uint8_t *out) {
  const pre::LensAs<MODEL> L(M);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      uint32_t v;
      if (!P)
        v = ch == 4 ? pre::rectify_px<4>(img, (size_t)cols * 4, rows, cols, L, x, y) : pre::rectify_px<1>(img, (size_t)cols, rows, cols, L, x, y);
      else if (P->bpp == 4)
        v = pre::rectify_source_px<4, false>(img, *P, L, x, y);
      else if (P->video)
        v = pre::rectify_source_px<1, true>(img, *P, L, x, y);
      else
        v = pre::rectify_source_px<1, false>(img, *P, L, x, y);
      out[(size_t)y * cols + x] = (uint8_t)v;
    }
}

static int write_out(const char *path, const void *p, size_t n) {
  FILE *f = fopen(path, "wb");
  return f && (n == 0 || fwrite(p, n, 1, f) == 1) && fclose(f) == 0 ? 0 : 7;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "layout")) {
    printf("%zu %zu %zu %zu\n", sizeof(VioLensModel), offsetof(VioLensModel, fx), offsetof(VioLensModel, k), offsetof(VioLensModel, rect_fx));
    return 0;
  }
  if (argc != 4) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 3;
  if (!strcmp(argv[1], "atan")) {
    std::vector<double> x;
    double v;
    while (fread(&v, sizeof v, 1, f) == 1) x.push_back(pre::lens_atan(v));
    fclose(f);
    return write_out(argv[3], x.data(), x.size() * sizeof(double));
  }
  if (strcmp(argv[1], "rectify")) return 2;
  int32_t hdr[4];
  VioLensModel M;
  VioSource S;
  if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(&M, sizeof M, 1, f) != 1) return 4;
  const int rows = hdr[0], cols = hdr[1], ch = hdr[2], has_source = hdr[3];
  if (has_source && fread(&S, sizeof S, 1, f) != 1) return 4;
  if (rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || !pre::lens_model_valid(M)) return 5;
  if (has_source ? !pre::source_valid(S, rows, cols) : !(ch == 1 || ch == 4)) return 5;
  const size_t bytes = has_source ? (size_t)S.rows * S.stride : (size_t)rows * cols * ch;
  std::vector<uint32_t> words((bytes + 3) / 4);  // 4-byte aligned, as the RGBA / BGRA read wants it
  uint8_t *img = reinterpret_cast<uint8_t *>(words.data());
  if (fread(img, bytes, 1, f) != 1) return 6;
  fclose(f);
  pre::SourcePlan plan;
  if (has_source) plan = pre::source_plan(S, rows, cols);
  const pre::SourcePlan *P = has_source ? &plan : nullptr;
  std::vector<uint8_t> out((size_t)rows * cols);
  if (M.model == VIO_LENS_FISHEYE)
    rectify<VIO_LENS_FISHEYE>(img, ch, rows, cols, M, P, out.data());
  else if (M.model == VIO_LENS_RATIONAL)
    rectify<VIO_LENS_RATIONAL>(img, ch, rows, cols, M, P, out.data());
  else
    rectify<VIO_LENS_BROWN>(img, ch, rows, cols, M, P, out.data());
  return write_out(argv[3], out.data(), out.size());
}
