// fe_track_update_body.inc -- the body of track_update_kernel (fe_track_update.h) behind its prologue, as text: the lock-step kernel
// and its subset instantiation (track_update_subset_kernel) include it, so that the lock-step kernel compiles from the token
// sequence it always had. The prologue provides: CAP, A, publish; T, R, seq, tid, nt.
  const size_t base = (size_t)seq * A.cap;
  const int n0 = A.n_pts[seq];
#define TU_STAMP(k)                                                  \
  do {                                                               \
    if (A.prof && seq == 0 && tid == 0) A.prof[k] = clock64();       \
  } while (0)
  TU_STAMP(0);
  if (tid == 0) T.n = n0;
  for (int i = tid; i < n0; i += nt) {
    T.pre[i][0] = A.pre_pts[(base + i) * 2], T.pre[i][1] = A.pre_pts[(base + i) * 2 + 1];
    T.cur[i][0] = A.cur_pts[(base + i) * 2], T.cur[i][1] = A.cur_pts[(base + i) * 2 + 1];
    T.forw[i][0] = A.forw_pts[(base + i) * 2], T.forw[i][1] = A.forw_pts[(base + i) * 2 + 1];
    T.ids[i] = A.ids[base + i], T.cnt[i] = A.track_cnt[base + i];
    // status && inBorder (feature_tracker.cpp:183-185, :18-24)
    int ix = __float2int_rn(T.forw[i][0]), iy = __float2int_rn(T.forw[i][1]);
    bool inb = 1 <= ix && ix < A.cols - 1 && 1 <= iy && iy < A.rows - 1;
    T.keep[i] = (A.lk_status[base + i] && inb) ? 1 : 0;
  }
  __syncthreads();
  TU_STAMP(1);
  shorten_list<CAP, true>(T);
  TU_STAMP(2);
  // The two F-tests share ONE inlined copy of the RANSAC code (the pass loop is kept a loop):
  //   pass 0  findFundamentalMat(cur_pts, forw_pts, FM_RANSAC, F_THRESHOLD, 0.99) :194-205
  //   pass 1  rejectWithF: (pre_pts, forw_pts) :89-103, publish frames only
  // Every condition below is uniform over the workgroup (T.n is read behind a barrier), so every barrier is reached by all.
  const int npass = publish ? 2 : 1;
#pragma nounroll
  for (int pass = 0; pass < npass; pass++) {
    if (pass) TU_STAMP(5);
    const int np = T.n;
    if (np >= 8) {
      // the list's correspondences side by side: the F-test reads position i with one LDS instruction and no index in between
      const float(*from)[2] = pass ? T.pre : T.cur;
      for (int i = tid; i < np; i += nt) {
        const int o = T.idx[i];
        T.pack[i] = make_float4(from[o][0], from[o][1], T.forw[o][0], T.forw[o][1]);
      }
      __syncthreads();
      fundamental_ransac_block(R, PackedPts{T.pack}, np, A.f_thresh, A.f_conf, T.keep, A.prof && seq == 0 ? A.prof + 16 + 8 * pass : nullptr);
      TU_STAMP(pass ? 6 : 3);
      shorten_list<CAP, false>(T);
    }
    if (pass == 0) {
      TU_STAMP(4);
      // the point list solveVinsPnP joins with the solved landmarks (:207): behind the first rejection, ahead of the
      // publish-frame steps (rejectWithF :235, setMask :255) that drop more of it
      for (int i = tid; i < T.n; i += nt) {
        const int o = T.idx[i];
        A.pnp_pts[(base + i) * 2] = T.forw[o][0], A.pnp_pts[(base + i) * 2 + 1] = T.forw[o][1];
        A.pnp_ids[base + i] = T.ids[o];
      }
      if (tid == 0) A.n_pnp[seq] = T.n;
    }
  }
  const int n = T.n;
  if (publish) {
    TU_STAMP(7);
    for (int i = tid; i < n; i += nt) {
      const int o = T.idx[i];
      T.ncnt[i] = T.cnt[o] + 1;  // for (auto &n : track_cnt) n++ :252-253
      T.ixy[i][0] = __float2int_rn(T.forw[o][0]), T.ixy[i][1] = __float2int_rn(T.forw[o][1]);
      if (REGION) {
        // the mask starts as the sequence's region: a position on a 0 pixel is never kept (and so never paints its disc). Its bit waits in
        // pos[], which the greedy pass writes for kept positions only, each behind its own decision. (inBorder: the pixel is in the image)
        int usable = 1;
        if (G.set[seq]) usable = (int)(region_window(G.words + ((size_t)seq * A.rows + T.ixy[i][1]) * G.wpr, G.wpr, T.ixy[i][0]) & 1ull);
        T.pos[i] = usable;
      }
    }
    __syncthreads();
    // setMask :50-87 — stable order by track_cnt desc (i, j below are list positions)
    for (int i = tid; i < n; i += nt) {
      int rank = 0, ci = T.ncnt[i];
      for (int j = 0; j < n; j++) rank += (T.ncnt[j] > ci || (T.ncnt[j] == ci && j < i)) ? 1 : 0;
      T.order[rank] = i;
    }
    const int words = (n + 63) / 64;
    __syncthreads();
    TU_STAMP(8);
    // inside[i][w] bit j: pixel of i lies in the filled circle painted at j (i, j: list positions, not ranks). One word per wave
    // instruction: the wave takes (i, w), lane b tests j = 64 w + b, the ballot IS the word. (The per-thread loop over
    // 64 j with the half-width table read from global memory inside it was 57 k cycles; the table now sits in LDS.)
    for (int q = tid; q < 2 * A.radius + 1; q += nt) T.hw[q] = A.hw[q];
    __syncthreads();
    {
      // lane b keeps the centres j = 64 w + b of the (at most kW) words in registers and walks i: per (i, w) two compares, one
      // table read and a ballot -- the item loop that re-read both centres per (i, w) was a chain of three dependent LDS round
      // trips per item (566 cycles each, 18 % of the kernel)
      const int wave = tid >> 6, lane = tid & 63, nwv = nt >> 6;
      constexpr int kW = CAP / 64;
      int jx[kW], jy[kW];
#pragma unroll
      for (int w = 0; w < kW; w++) {
        const int j = min(64 * w + lane, n - 1);
        jx[w] = T.ixy[j][0], jy[w] = T.ixy[j][1];
      }
      const int rad = A.radius;
      for (int i = wave; i < n; i += nwv) {
        const int ix = T.ixy[i][0], iy = T.ixy[i][1];
#pragma unroll
        for (int w = 0; w < kW; w++) {
          if (w < words) {
            const int dy = iy - jy[w], dx = ix - jx[w];
            const int h = T.hw[rad + min(max(dy, -rad), rad)];
            const bool in = 64 * w + lane < n && dy >= -rad && dy <= rad && dx >= -h && dx <= h;
            const unsigned long long bits = __builtin_amdgcn_ballot_w64(in);
            if (lane == 0) T.inside[i][w] = bits;
          }
        }
      }
    }
    __syncthreads();
    TU_STAMP(9);
    // greedy in sorted order (:73-83): a feature is kept unless it lies in the circle of an earlier kept one. One wave:
    // lane w owns word w of the kept set in a register, the hit test is a ballot; the index list and the bit rows do not
    // depend on the decisions, so the compiler is free to fetch them ahead. Kept features get their output position
    // (forw_pts.push_back order) on the way. (One thread with the kept set in a dynamically indexed array: 105 k cycles.)
    if (tid < 64) {
      const int lane = tid;
      unsigned long long mine = 0;  // word `lane` of the kept set
      int c = 0;
      for (int r0 = 0; r0 < n; r0 += 64) {
        const int my_i = r0 + lane < n ? T.order[r0 + lane] : 0;
        const int cnt = n - r0 < 64 ? n - r0 : 64;
        const unsigned long long usable = REGION ? __builtin_amdgcn_ballot_w64(r0 + lane < n && T.pos[my_i] != 0) : ~0ull;  // bit q: candidate r0 + q lies on a usable pixel
        unsigned long long kept = 0;  // bit q: candidate r0 + q is kept (uniform)
        for (int q0 = 0; q0 < cnt; q0 += 8) {  // the bit rows of eight candidates are fetched together, then decided in order
          int is[8];
          unsigned long long rows[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            is[u] = __builtin_amdgcn_readlane(my_i, (q0 + u) & 63);
            rows[u] = lane < words ? T.inside[is[u]][lane] : 0ull;
          }
#pragma unroll
          for (int u = 0; u < 8; u++) {  // (no LDS traffic and no lane-0 branches inside the chain: the decisions go to a bit mask)
            const int i = is[u];
            const bool keep_it = q0 + u < cnt && (!REGION || ((usable >> ((q0 + u) & 63)) & 1ull)) && __builtin_amdgcn_ballot_w64((rows[u] & mine) != 0) == 0;
            const unsigned long long bit = keep_it ? 1ULL << (i & 63) : 0ull;
            mine |= lane == (i >> 6) ? bit : 0ull;
            kept |= (unsigned long long)keep_it << ((q0 + u) & 63);
          }
        }
        if (lane < cnt) {  // candidate r0 + lane: its decision and, if kept, its output position (forw_pts.push_back order)
          const bool k = (kept >> lane) & 1ull;
          T.keep[my_i] = k ? 1 : 0;
          if (k) T.pos[my_i] = c + __builtin_popcountll(kept & ((1ull << lane) - 1ull));
        }
        c += __builtin_popcountll(kept);
      }
      if (lane == 0) T.n = c;
    }
    __syncthreads();
    TU_STAMP(10);
    // the arrays are gathered once, here, straight into the tracker's fields: list position i -> slot idx[i] -> output position pos[i]
    // (forw_pts.push_back order); pre_pts / cur_pts are overwritten with forw_pts at the end of a publish frame (:274, :285)
    for (int i = tid; i < n; i += nt)
      if (T.keep[i]) {
        const int p = T.pos[i], o = T.idx[i];
        A.forw_pts[(base + p) * 2] = T.forw[o][0], A.forw_pts[(base + p) * 2 + 1] = T.forw[o][1];
        A.ids[base + p] = T.ids[o], A.track_cnt[base + p] = T.ncnt[i];
        A.kept_xy[(base + p) * 2] = T.ixy[i][0], A.kept_xy[(base + p) * 2 + 1] = T.ixy[i][1];
      }
    if (tid == 0) A.n_kept[seq] = T.n, A.n_forw[seq] = T.n;
  } else {
    for (int i = tid; i < n; i += nt) {
      const int o = T.idx[i];
      A.forw_pts[(base + i) * 2] = T.forw[o][0], A.forw_pts[(base + i) * 2 + 1] = T.forw[o][1];
      A.ids[base + i] = T.ids[o], A.track_cnt[base + i] = T.cnt[o];
      A.pre_pts[(base + i) * 2] = T.pre[o][0], A.pre_pts[(base + i) * 2 + 1] = T.pre[o][1];
      // cur_pts = forw_pts (:285)
      A.cur_pts[(base + i) * 2] = T.forw[o][0], A.cur_pts[(base + i) * 2 + 1] = T.forw[o][1];
    }
    if (tid == 0) A.n_forw[seq] = n, A.n_pts[seq] = n;
  }
  TU_STAMP(11);
#undef TU_STAMP
