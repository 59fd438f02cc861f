// fe_pyr_down_body.inc -- the body of pyr_down_kernel (fe_pyramid.h) behind its prologue, as text, shared with pyr_down_subset_kernel
// so that the lock-step kernel compiles from the token sequence it always had. The prologue provides: SW, SH, patch, hsum, src, dst and
// the kernel's srows .. dcols.
  const int ox = blockIdx.x * kPdW, oy = blockIdx.y * kPdH;
  const int tid = threadIdx.x;
  for (int e = tid; e < SH * SW; e += 256) {
    int ly = e / SW, lx = e - ly * SW;
    int y = reflect101(min(2 * oy + ly - 2, 2 * srows - 2), srows), x = reflect101(min(2 * ox + lx - 2, 2 * scols - 2), scols);
    patch[ly][lx] = src[(size_t)y * scols + x];
  }
  __syncthreads();
  for (int e = tid; e < SH * kPdW; e += 256) {
    int ly = e / kPdW, lx = e - ly * kPdW;
    const int *r = &patch[ly][2 * lx];
    hsum[ly][lx] = r[0] + 4 * r[1] + 6 * r[2] + 4 * r[3] + r[4];
  }
  __syncthreads();
  for (int e = tid; e < kPdH * kPdW; e += 256) {
    int ly = e / kPdW, lx = e - ly * kPdW;
    int x = ox + lx, y = oy + ly;
    if (x < dcols && y < drows) {
      int v = hsum[2 * ly][lx] + 4 * hsum[2 * ly + 1][lx] + 6 * hsum[2 * ly + 2][lx] + 4 * hsum[2 * ly + 3][lx] + hsum[2 * ly + 4][lx];
      dst[(size_t)y * dcols + x] = (uint8_t)((v + 128) >> 8);
    }
  }
