// fe_lk_body.inc -- the body of lk_track_kernel (fe_lk.h) behind its prologue, as text: the lock-step kernel and its subset
// instantiation (lk_track_subset_kernel) include it, so that the lock-step kernel compiles from the token sequence it always had.
// The prologue provides: STATS, ERR, P, n_pts .. stats as in lk_track_kernel; seq, wave, lane, pt, L, pp, np, pidx.
  const float ptx = prev_pts[pidx], pty = prev_pts[pidx + 1];
  const float half = (kWin - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (1 << 20);
  constexpr int NPX = (kWin * kWin + 63) / 64;  // window pixels per lane: 7
  // This lane's window pixels (lk_layout.h): seven consecutive rows wy0 + q (q = 0..6) of column wx0 -- the q-th pixel sits a
  // CONSTANT q rows below the first, so the LDS reads of an iteration share one address register (+ immediate offsets)
  // instead of one address computation per pixel. (The sums over the window are exact integers: which lane owns which pixel
  // does not reach the result.)
  static_assert(NPX == lk_layout::kPxPerLane, "pixels per lane");
  const lk_layout::Px px0 = lk_layout::lane_pixel0(lane);
  const int wy0 = px0.row, wx0 = px0.col;  // (lane 63 owns nothing: it shadows lane 42's addresses, masked below)
  const int joff = wy0 * kJS + wx0;  // element offset of the first pixel in the staged J region
  bool st = true;
  float er = 0.f;
  float nxx = 0.f, nxy = 0.f;
  const int max_level = P.ld.levels - 1;
  for (int level = max_level; level >= 0; level--) {
    const int rows = P.ld.rows[level], cols = P.ld.cols[level];
    const uint8_t *I = pp + P.ld.off[level], *J = np + P.ld.off[level];
    if (level == 0) {  // (scalar selects)
      if (P.prev0) I = P.prev0 + (size_t)seq * P.stride0;
      if (P.next0) J = P.next0 + (size_t)seq * P.stride0;
    }
    const float scale = __int_as_float((127 - level) << 23);  // (float)(1. / (1 << level)) = 2^-level, without the double division
    float px = ptx * scale, py = pty * scale;
    float qx, qy;
    if (level == max_level) qx = px, qy = py;
    else qx = nxx * 2.f, qy = nxy * 2.f;
    nxx = qx, nxy = qy;
    px -= half, py -= half;
    int ipx = (int)floorf(px), ipy = (int)floorf(py);
    if (ipx < -kWin || ipx >= cols || ipy < -kWin || ipy >= rows) {
      if (level == 0) st = false, er = 0.f;
      continue;
    }
    float a = px - ipx, b = py - ipy;
    int iw00, iw01, iw10, iw11;
    lk_weights(a, b, iw00, iw01, iw10, iw11);
    // stage I on [ipx-1, ipx+23) x [ipy-1, ipy+23) (BORDER_REFLECT_101), then its Scharr derivatives on
    // [ipx, ipx+22) x [ipy, ipy+22): zero outside the image (copyMakeBorder BORDER_CONSTANT of derivI)
    wave_lds_fence();  // previous level's readers are done
    if (ipx >= 1 && ipx + kIP - 1 <= cols && ipy >= 1 && ipy + kIP - 1 <= rows) {
      // the patch lies inside the image (all but the features within a window of the border): FOUR pixels per lane and
      // load, 6 lanes per row, 10 rows per trip -- 3 trips instead of 12 (the kernel is VALU-issue-bound: staging the two
      // patches byte by byte was a quarter of a level's instructions)
      const int r = lane / 6, d = lane - 6 * r;
      constexpr int TI = (kIP + 9) / 10;
      uint32_t curs[TI];
#pragma unroll
      for (int t = 0; t < TI; t++) {  // (the loads of all trips in flight together: one global round trip per patch, not one per trip)
        const int ly = r + 10 * t;
        curs[t] = lk_load4(I + (unsigned)(__mul24(ipy - 1 + (ly < kIP ? ly : 0), cols) + ipx - 1 + 4 * d));
      }
#pragma unroll
      for (int t = 0; t < TI; t++) {  // (uniform trip count: the DPP below needs every lane)
        const int ly = r + 10 * t;
        const bool ok = lane < 60 && ly < kIP;
        const uint32_t cur = curs[t];
        uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cur, 0x130, 0xf, 0xf, false);  // dword of lane + 1
        if (d == 5) next = cur >> 24;  // (the pair behind the last pixel repeats it, like the byte path's clamped lane)
        uint32_t w4[4];
        lk_pairs(cur, next, w4);
        if (ok) {
#pragma unroll
          for (int k = 0; k < 4; k++) L.I[ly][4 * d + k] = w4[k];
        }
      }
    } else {  // 32 lanes per row (24 used), two rows per trip: the column index is reflected once per lane; the right-hand
       // neighbour of every pixel comes from the next lane (DPP wave_shl) so that a pair can be stored as one dword
      const int lx = lane & 31;
      const int x = reflect101(ipx - 1 + min(lx, kIP - 1), cols);
      // (a third of the features take this path at the coarse levels, where the patch is a quarter of the image: all loads
      // of the patch are issued before the first is consumed -- one memory round trip instead of one per trip)
      constexpr int RPT = 2, TB = kIP / RPT;
      static_assert(kIP % RPT == 0, "whole trips");
      int vs[TB];
#pragma unroll
      for (int t = 0; t < TB; t++) {
        // (the patch origin is the same in every lane, so the reflected ROW of a trip is one of two scalars -- even / odd half
        // of the wave -- and comes off the scalar unit: 2 vector instructions per trip instead of ~16; the border path is not
        // rare: 58 % of the features take it at level 3, 32 % at level 2)
        const int s_y0 = __builtin_amdgcn_readfirstlane(ipy) - 1 + RPT * t;
        const int ro_a = reflect101(s_y0, rows) * cols, ro_b = reflect101(s_y0 + 1, rows) * cols;
        vs[t] = I[(unsigned)(((lane >> 5) ? ro_b : ro_a) + x)];
      }
#pragma unroll
      for (int t = 0; t < TB; t++) {
        const int ly = (lane >> 5) + RPT * t, v = vs[t];
        const int vr = __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false);  // value of lane + 1
        if (lx < kIP) L.I[ly][lx] = (uint32_t)v | ((uint32_t)vr << 16);
      }
    }
    wave_lds_fence();
    // Scharr derivatives by COLUMN-PAIR WALK on packed 16-bit arithmetic: lanes 0..54 = 11 column pairs x five segments of five
    // output rows (the last one starts at row 17 and repeats three rows of its neighbour). A staged dword is a pixel pair
    // (I[x] | I[x+1] << 16), so the three pair words at columns c, c + 1, c + 2 are the left / centre / right taps of the derivative
    // columns c AND c + 1 at once: per input row h = P2 - P0 and v = 3 (P0 + P2) + 10 P1, per output row dx = 3 (h0 + h2) + 10 h1 and
    // dy = v2 - v0, each ONE v_pk_* instruction for both columns (|values| <= 16 x 255: exact in 16 bits) -- the same integers as the
    // 3 x 3 sums of calcSharrDeriv. (The one-column walk on 32-bit values, rounds 4-6: 168 vector instructions per level on 44 lanes,
    // a seventh of the kernel's; this form: ~75 on 55 lanes.)
    constexpr int SEG = 5, NSEG = 5, NCP = kDP / 2;
    static_assert(kDP % 2 == 0 && NCP * NSEG <= 64 && SEG * NSEG >= kDP && kDP >= SEG, "column pairs x segments");
    const bool inside = ipx >= 0 && ipx + kDP <= cols && ipy >= 0 && ipy + kDP <= rows;  // every derivative position is in the image
    if (lane < NCP * NSEG) {
      const int seg = lane / NCP, cp = lane - NCP * seg, c = 2 * cp;
      const int r0 = seg * SEG < kDP - SEG ? seg * SEG : kDP - SEG;
      const uint32_t *Ip = &L.I[0][0] + (__mul24(r0, kIS) + c);
      uint32_t *Dp = reinterpret_cast<uint32_t *>(&L.dI[0][0]) + (__mul24(r0, kDS) + c);
      const lk_s2 k3 = {3, 3}, k10 = {10, 10};
      auto walk = [&](auto checked) {  // (checked: the patch leaves the image -- derivI's BORDER_CONSTANT zeros)
        const unsigned ok0 = (unsigned)(ipx + c) < (unsigned)cols, ok1 = (unsigned)(ipx + c + 1) < (unsigned)cols;
        lk_s2 P0[SEG + 2], P1[SEG + 2], P2[SEG + 2];  // pair words of input row r0 + r: the staged patch holds reflected values at the image border
#pragma unroll
        for (int r = 0; r < SEG + 2; r++)  // (all reads ahead of the first write: one wait instead of one per row)
          __builtin_memcpy(&P0[r], Ip + r * kIS, 4), __builtin_memcpy(&P1[r], Ip + r * kIS + 1, 4), __builtin_memcpy(&P2[r], Ip + r * kIS + 2, 4);
        lk_s2 h[SEG + 2], v[SEG + 2];
#pragma unroll
        for (int r = 0; r < SEG + 2; r++) h[r] = P2[r] - P0[r], v[r] = (P0[r] + P2[r]) * k3 + P1[r] * k10;
#pragma unroll
        for (int r = 2; r < SEG + 2; r++) {
          const lk_s2 dx = (h[r - 2] + h[r]) * k3 + h[r - 1] * k10, dy = v[r] - v[r - 2];
          uint32_t ux, uy;
          __builtin_memcpy(&ux, &dx, 4), __builtin_memcpy(&uy, &dy, 4);
          uint32_t d0 = __builtin_amdgcn_perm(uy, ux, 0x05040100u), d1 = __builtin_amdgcn_perm(uy, ux, 0x07060302u);  // short2 {dx, dy} of columns c, c + 1
          if (decltype(checked)::value) {
            const unsigned rok = (unsigned)(ipy + r0 + r - 2) < (unsigned)rows;
            d0 &= 0u - (ok0 & rok), d1 &= 0u - (ok1 & rok);
          }
          Dp[(r - 2) * kDS] = d0, Dp[(r - 2) * kDS + 1] = d1;
        }
      };
      if (inside) walk(std::false_type{});
      else walk(std::true_type{});
    }
    wave_lds_fence();
    // template patch + derivatives for this lane's window pixels, kept in registers across the iterations
    // (the template value enters the iterations as the accumulator seed of the bilinear sample: rounding constant minus
    // Iv << n, so that the arithmetic shift that ends the sample yields J - I directly -- (a + r - (Iv << n)) >> n ==
    // ((a + r) >> n) - Iv exactly)
    // Ix, Iy of pixels 2h and 2h + 1 share a register: the iterations multiply-accumulate them pairwise (v_dot2_i32_i16).
    constexpr int NPP = (NPX + 1) / 2;
    const lk_s2 sw_top = {(short)iw00, (short)iw01}, sw_bot = {(short)iw10, (short)iw11};
    lk_s2 IxP[NPP], IyP[NPP];
    int Ic[NPX];
    int p11 = 0, p12 = 0, p22 = 0;  // per-lane partials: <= 14 products of |v| <= 4080^2 fit 32 bits
#pragma unroll
    for (int h = 0; h < NPP; h++) IxP[h] = IyP[h] = lk_s2{0, 0};
    // bilinear taps as dot products of packed pairs (a 32-bit integer multiply is a quarter-rate instruction here; the
    // element-wise form of this block was 12 of them per pixel): the I patch is staged as pairs already; the derivative
    // pairs (d[x], d[x+1]) are cut out of two (dx, dy) words with v_perm_b32. Weights <= 2^14 fit int16, and the SIGNED
    // dot keeps iw11 = 2^14 - iw00 - iw01 - iw10 right when the three roundings push it to -1.
    // The lane's pixels are consecutive rows of one column: the bottom row words of pixel q are the top row words of pixel
    // q + 1, read (and cut) once -- 8 reads of I and 16 of dI per lane instead of 14 and 28.
    const uint32_t *Iw = &L.I[wy0 + 1][wx0 + 1], *Dw = &L.dI[wy0][wx0];  // (I[x+1], I[x+2]) of row y + 1; (dx, dy) of [y][x]
    auto tap_row = [&](int k, lk_s2 &iv, lk_s2 &sx, lk_s2 &sy) {
      uint32_t d0, d1;
      __builtin_memcpy(&iv, Iw + k * kIS, 4);
      __builtin_memcpy(&d0, Dw + k * kDS, 4), __builtin_memcpy(&d1, Dw + k * kDS + 1, 4);
      const uint32_t xs = __builtin_amdgcn_perm(d1, d0, 0x05040100u), ys = __builtin_amdgcn_perm(d1, d0, 0x07060302u);
      __builtin_memcpy(&sx, &xs, 4), __builtin_memcpy(&sy, &ys, 4);
    };
    lk_s2 it, sxt, syt;
    tap_row(0, it, sxt, syt);
#pragma unroll
    for (int q = 0; q < NPX; q++) {  // (rows wy0 + q: always inside the window)
      lk_s2 ib, sxb, syb;
      tap_row(q + 1, ib, sxb, syb);
      const int ival = __builtin_amdgcn_sdot2(it, sw_top, __builtin_amdgcn_sdot2(ib, sw_bot, 1 << (kWBits - 5 - 1), false), false) >> (kWBits - 5);
      int ixval = __builtin_amdgcn_sdot2(sxt, sw_top, __builtin_amdgcn_sdot2(sxb, sw_bot, 1 << (kWBits - 1), false), false) >> kWBits;
      int iyval = __builtin_amdgcn_sdot2(syt, sw_top, __builtin_amdgcn_sdot2(syb, sw_bot, 1 << (kWBits - 1), false), false) >> kWBits;
      it = ib, sxt = sxb, syt = syb;
      if (lane >= 3 * kWin) ixval = iyval = 0;  // a pixel this lane does not own: weight zero in every sum below
      Ic[q] = (1 << (kWBits - 5 - 1)) - (int)((unsigned)ival << (kWBits - 5));
      if (q & 1) IxP[q >> 1].y = (short)ixval, IyP[q >> 1].y = (short)iyval;
      else IxP[q >> 1].x = (short)ixval, IyP[q >> 1].x = (short)iyval;
      p11 += ixval * ixval, p12 += ixval * iyval, p22 += iyval * iyval;
    }
    float f11, f12, f22;  // exact integer sums, rounded once to float
    wave_sum_exact3(p11, p12, p22, f11, f12, f22);
    float A11 = f11 * FLT_SCALE, A12 = f12 * FLT_SCALE, A22 = f22 * FLT_SCALE;
    float D = A11 * A22 - A12 * A12;
    float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * kWin * kWin);
    if (minEig < P.min_eig || D < 1.1920929e-07f) {
      if (level == 0) st = false;
      continue;
    }
    D = 1.f / D;
    qx -= half, qy -= half;
    float pdx = 0.f, pdy = 0.f;
    int jox = 0, joy = 0;      // origin of the staged J region
    bool j_staged = false;
    auto stage_j = [&](int iqx, int iqy) {
      jox = iqx - kJMargin, joy = iqy - kJMargin;
      wave_lds_fence();
      if (jox >= 0 && jox + kJP <= cols && joy >= 0 && joy + kJP <= rows) {
        // inside the image: 4 pixels per lane and load, 7 lanes per row, 9 rows per trip -- 4 trips instead of 14
        const int r = lane / 7, d = lane - 7 * r;
        constexpr int TJ = (kJP + 8) / 9;
        uint32_t curs[TJ];
#pragma unroll
        for (int t = 0; t < TJ; t++) {
          const int ly = r + 9 * t;
          curs[t] = lk_load4(J + (unsigned)(__mul24(joy + (ly < kJP ? ly : 0), cols) + jox + 4 * d));
        }
#pragma unroll
        for (int t = 0; t < TJ; t++) {
          const int ly = r + 9 * t;
          const bool ok = lane < 63 && ly < kJP;
          const uint32_t cur = curs[t];
          uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cur, 0x130, 0xf, 0xf, false);
          if (d == 6) next = cur >> 24;
          uint32_t w4[4];
          lk_pairs(cur, next, w4);
          if (ok) {
#pragma unroll
            for (int k = 0; k < 4; k++) L.J[ly][4 * d + k] = w4[k];
          }
        }
      } else {  // 32 lanes per row (28 used), two rows per trip; pairs (J[x] | J[x+1] << 16) like the template patch
        const int lx = lane & 31;
        const int x = reflect101(min(max(jox + min(lx, kJP - 1), -cols + 1), 2 * cols - 2), cols);
        constexpr int RPT = 2, TB = kJP / RPT;
        static_assert(kJP % RPT == 0, "whole trips");
        int vs[TB];
#pragma unroll
        for (int t = 0; t < TB; t++) {  // (rows on the scalar unit, as in the template patch's border path)
          const int s_y0 = __builtin_amdgcn_readfirstlane(joy) + RPT * t;
          const int ro_a = reflect101(min(max(s_y0, -rows + 1), 2 * rows - 2), rows) * cols;
          const int ro_b = reflect101(min(max(s_y0 + 1, -rows + 1), 2 * rows - 2), rows) * cols;
          vs[t] = J[(unsigned)(((lane >> 5) ? ro_b : ro_a) + x)];
        }
#pragma unroll
        for (int t = 0; t < TB; t++) {
          const int ly = (lane >> 5) + RPT * t, v = vs[t];
          const int vr = __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false);  // value of lane + 1
          if (lx < kJP) L.J[ly][lx] = (uint32_t)v | ((uint32_t)vr << 16);
        }
      }
      wave_lds_fence();
      j_staged = true;
    };
    const uint32_t *Jl = &L.J[0][0];
    // (the top-row weights are never negative: their dot is the unsigned three-operand instruction, seeded with Ic without
    // a copy; the bottom row, whose iw11 can be -1, goes through the signed accumulate-in-place one)
    // (the pair words of the lane's eight rows, each read once: row q + 1 is the bottom of pixel q and the top of pixel q + 1)
    auto load_j = [&](int base, uint32_t (&jr)[NPX + 1]) {
#pragma unroll
      for (int k = 0; k <= NPX; k++) jr[k] = Jl[base + (joff + k * kJS)];  // (one address register + immediate offsets)
    };
    auto diff_j = [&](const uint32_t (&jr)[NPX + 1], int q, lk_us2 wtop, lk_s2 wbot) {  // bilinear J at this lane's q-th window pixel, minus I there
      lk_us2 top;
      lk_s2 bot;
      __builtin_memcpy(&top, &jr[q], 4);
      __builtin_memcpy(&bot, &jr[q + 1], 4);
      return __builtin_amdgcn_sdot2(bot, wbot, (int)__builtin_amdgcn_udot2(top, wtop, (unsigned)Ic[q], false), false) >> (kWBits - 5);  // (mod 2^32)
    };
    int nit = 0;  // (STATS only)
    for (int j = 0; j < P.max_count; j++) {
      int iqx = (int)floorf(qx), iqy = (int)floorf(qy);
      if (iqx < -kWin || iqx >= cols || iqy < -kWin || iqy >= rows) {
        if (level == 0) st = false;
        break;
      }
      if (STATS) nit++;
      if (!j_staged || iqx < jox || iqx > jox + 2 * kJMargin || iqy < joy || iqy > joy + 2 * kJMargin) stage_j(iqx, iqy);
      a = qx - iqx, b = qy - iqy;
      lk_weights(a, b, iw00, iw01, iw10, iw11);
      int pb1 = 0, pb2 = 0;  // |diff * dI| <= 16320 * 4080 per pixel, <= 14 pixels per lane: 9.3e8 fits 32 bits
      const lk_us2 wtop = {(unsigned short)iw00, (unsigned short)iw01};
      const lk_s2 wbot = {(short)iw10, (short)iw11};
      const int jbase = __mul24(iqy - joy, kJS) + (iqx - jox);
      uint32_t jr[NPX + 1];
      load_j(jbase, jr);
#pragma unroll
      for (int h = 0; h < NPP; h++) {  // (a pixel the lane does not own has Ix = Iy = 0)
        const int d0 = diff_j(jr, 2 * h, wtop, wbot), d1 = 2 * h + 1 < NPX ? diff_j(jr, 2 * h + 1, wtop, wbot) : 0;
        const unsigned pk = __builtin_amdgcn_perm((unsigned)d1, (unsigned)d0, 0x05040100u);  // |J - I| <= 8160: (d0, d1) as two int16
        lk_s2 dp;
        __builtin_memcpy(&dp, &pk, 4);
        pb1 = __builtin_amdgcn_sdot2(dp, IxP[h], pb1, false), pb2 = __builtin_amdgcn_sdot2(dp, IyP[h], pb2, false);
      }
      float fb1, fb2;  // the exact integer sums, rounded once to float (what (float) of the exact double gave)
      wave_sum_exact2(pb1, pb2, fb1, fb2);
      float b1 = fb1 * FLT_SCALE, b2 = fb2 * FLT_SCALE;
      float ddx = (A12 * b2 - A22 * b1) * D, ddy = (A12 * b1 - A11 * b2) * D;
      qx += ddx, qy += ddy;
      nxx = qx + half, nxy = qy + half;
      // delta.ddot(delta) <= epsilon in double, behind a float screen that only lets candidates through (conversions to and
      // from double are slow instructions; all but the last iteration of a level stop at the screen)
      if (!(ddx * ddx + ddy * ddy > P.epsilon_sq_f) && (double)ddx * ddx + (double)ddy * ddy <= P.epsilon_sq) break;
      // |x| < 0.01 for a float x: 0.01 (double) lies strictly between 0.01f and the next float up, so the float compare against
      // that next float decides the same
      constexpr float kCentiUp = 0.010000000707805157f;
      static_assert((double)kCentiUp > 0.01 && (double)0.01f < 0.01, "float neighbours of 0.01");
      if (j > 0 && fabsf(ddx + pdx) < kCentiUp && fabsf(ddy + pdy) < kCentiUp) {
        nxx -= ddx * 0.5f, nxy -= ddy * 0.5f;
        break;
      }
      pdx = ddx, pdy = ddy;
    }
    if (STATS && lane == 0) {  // (64 copies of the counters, picked by block: one address would serialize every wave of the launch)
      unsigned long long *sl = stats + ((blockIdx.x + 7 * blockIdx.y) & 63) * 16;
      atomicAdd(sl + level, (unsigned long long)nit);
      atomicAdd(sl + P.ld.levels + level, 1ull);
    }
    if (st && level == 0) {
      float ex = nxx - half, ey = nxy - half;
      int iex = (int)floorf(ex), iey = (int)floorf(ey);
      if (iex < -kWin || iex >= cols || iey < -kWin || iey >= rows) {
        st = false;
        continue;
      }
      if (!ERR) continue;  // (the range test above is the status' last word: it stays)
      if (!j_staged || iex < jox || iex > jox + 2 * kJMargin || iey < joy || iey > joy + 2 * kJMargin) stage_j(iex, iey);
      float aa = ex - iex, bb = ey - iey;
      lk_weights(aa, bb, iw00, iw01, iw10, iw11);
      int pe = 0;
      const lk_us2 wtop = {(unsigned short)iw00, (unsigned short)iw01};
      const lk_s2 wbot = {(short)iw10, (short)iw11};
      const int jbase = __mul24(iey - joy, kJS) + (iex - jox);
      uint32_t jr[NPX + 1];
      load_j(jbase, jr);
#pragma unroll
      for (int q = 0; q < NPX; q++) {
        const int d = abs(diff_j(jr, q, wtop, wbot));
        pe += lane < 3 * kWin ? d : 0;
      }
      const int se = wave_sum_i32(pe);  // <= 441 * 16320 < 2^23
      er = (float)se * 1.f / (32 * kWin * kWin);
    }
  }
  if (lane == 0) {
    next_pts[pidx] = nxx, next_pts[pidx + 1] = nxy;
    status[(size_t)seq * P.cap + pt] = st ? 1 : 0;
    if (ERR) err[(size_t)seq * P.cap + pt] = er;
  }
