// tests/emul/simt_cameras.cpp — TEST-ONLY: the passes of the landmark store that read a camera (store_ingest with its
// triangulation, store_keyframe; vins-mobile_amd/csrc/store_core.h) executed on the host by the SIMT emulator for THREE slots
// that each carry their own camera, the way the kernels of vio_store.hip run them: the slot's camera -> body record through
// store::slot_camera out of one table of records, the job's intrinsics through store::job_intrinsics out of one table of rows.
// Every buffer starts NaN-poisoned. Each slot is compared, bit for bit, with the host-side list (vio_window.cpp) driven with
// that slot's camera: vio_features_triangulate and vio_features_keyframe. The caller (tests/test_cameras_emul.py) passes the
// cameras in slot order and the order of the keyframe jobs. Not part of the product library.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <stdarg.h>

#include <limits>
#include <random>
#include <vector>

#include "store_core.h"

#include "../../vins-mobile_amd/csrc/vio_window.cpp"

using namespace vio;
namespace st = vio::store;

namespace {

struct Msg {
  char *buf;
  int cap, n = 0, fails = 0;
  void add(const char *fmt, ...) {
    fails++;
    if (n >= cap - 1) return;
    va_list ap;
    va_start(ap, fmt);
    n += vsnprintf(buf + n, cap - n, fmt, ap);
    va_end(ap);
    if (n < cap - 1) buf[n++] = '\n', buf[n] = 0;
  }
};

const double kNan = std::numeric_limits<double>::quiet_NaN();

struct SimStore {  // one slot: two banks, control block, LDS
  st::Dims d;
  std::vector<int> fid[2], start[2], nobs[2], flag[2], ctl;
  std::vector<double> depth[2], obs[2];
  std::vector<int> lds_words;
  SimStore(int W, int Lcap, int Ocap) {
    d.W = W, d.Lcap = Lcap, d.Ocap = Ocap;
    for (int b = 0; b < 2; b++) {
      fid[b].assign(Lcap, -7), start[b].assign(Lcap, -7), nobs[b].assign(Lcap, -7), flag[b].assign(Lcap, -7);
      depth[b].assign(Lcap, kNan), obs[b].assign((size_t)Lcap * (W + 1) * 3, kNan);
    }
    ctl.assign(st::C_COUNT, 0);
    lds_words.assign(st::lds_bytes(d) / sizeof(int) + 16, -1);
  }
  st::Bank bank(int b) { return st::Bank{fid[b].data(), start[b].data(), nobs[b].data(), flag[b].data(), depth[b].data(), obs[b].data()}; }
  st::Lds lds() {
    double *dbase;
    std::fill(lds_words.begin(), lds_words.end(), -1);  // nothing survives in LDS from one launch to the next
    return st::carve_lds<int *, double *>(d, lds_words.data(), &dbase);
  }
};

constexpr int kSlots = 3, kRec = 19;  // a record as the back end lays it out: ex_pose 7 | tic 3 | ric 9

}  // namespace

// cams [3][16]: fx fy cx cy | tic 3 | ric 9 of the camera of slot 0, 1, 2. jobs [3]: the slot of keyframe job 0, 1, 2.
// shift: 0; otherwise the store side takes the record of slot (s + shift) % 3 and the row of job (j + shift) % 3 -- the wrong index
// the comparison has to see. Returns the number of mismatches (0 = identical); the first ones are described in msg.
// stats [3][2]: per slot the landmarks that carry a triangulated depth after the ingest, and the keyframe features.
extern "C" int simt_cameras(int seed, int W, int order, int shift, const double *cams, const int *jobs, char *msg_buf, int msg_cap, long long *stats) {
  Msg msg{msg_buf, msg_cap};
  if (msg_cap > 0) msg_buf[0] = 0;
  const int P = W + 1, Lcap = 1024, Ocap = 512, n_landmarks = 260, cap = 512;
  // the tables the kernels index: poisoned, then one record / one row per slot (ex_pose is not read by the store passes: it stays NaN)
  std::vector<double> consts((size_t)kSlots * kRec + 18, kNan), intr((size_t)kSlots * 4, kNan);
  for (int s = 0; s < kSlots; s++) {
    memcpy(&consts[(size_t)s * kRec + 7], cams + 16 * s + 4, sizeof(double) * 3);
    memcpy(&consts[(size_t)s * kRec + 10], cams + 16 * s + 7, sizeof(double) * 9);
  }
  for (int j = 0; j < kSlots; j++) memcpy(&intr[4 * (size_t)j], cams + 16 * jobs[j], sizeof(double) * 4);
  const double *tic0 = consts.data() + 7, *ric0 = consts.data() + 10;
  // (a stride of 0 is one shared record, no table of rows is the launch's own four: what a context without cameras runs)
  if (st::slot_camera(tic0, ric0, 0, 2).tic != tic0 || st::slot_camera(tic0, ric0, 0, 2).ric != ric0) msg.add("cam_stride 0 is not the shared record");
  {
    const st::Intrinsics in = st::job_intrinsics(nullptr, 2, 1.0, 2.0, 3.0, 4.0);
    if (in.fx != 1.0 || in.fy != 2.0 || in.cx != 3.0 || in.cy != 4.0) msg.add("a null table of intrinsics does not give the launch's own");
  }

  std::vector<SimStore> stores;
  std::vector<vio_features_t *> fms(kSlots, nullptr);
  std::vector<std::vector<double>> Ps(kSlots), Rs(kSlots);
  for (int s = 0; s < kSlots; s++) stores.emplace_back(W, Lcap, Ocap);
  for (int s = 0; s < kSlots; s++) {
    const double *tic = cams + 16 * s + 4, *ric = cams + 16 * s + 7;
    std::mt19937_64 rng(seed * 131 + s);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(rng() >> 11) / 9007199254740992.0; };
    // a scene of its own per slot: the body drifts along x and looks, through the slot's camera, at landmarks on both sides of z
    std::vector<double> lm(3 * (size_t)n_landmarks);
    for (int i = 0; i < n_landmarks; i++) lm[3 * i] = uni(-6, 12), lm[3 * i + 1] = uni(-5, 5), lm[3 * i + 2] = (i & 1 ? 1 : -1) * uni(3, 11);
    auto pose_at = [&](int k, double Pk[3], double Rk[9]) {
      Pk[0] = 0.13 * k + 0.01 * sin(0.7 * k + s), Pk[1] = 0.05 * sin(0.3 * k), Pk[2] = 0.02 * cos(0.5 * k);
      const double ypr[3] = {3.0 * sin(0.1 * k + s), 1.5 * cos(0.17 * k), 2.0 * sin(0.21 * k)};
      ypr2R(ypr, Rk);
    };
    auto observe = [&](int k, std::vector<VioObs> &out) {
      out.clear();
      double Pk[3], Rk[9], Rc[9], RcT[9], tc[3], tmp[3];
      pose_at(k, Pk, Rk);
      mat3mul(Rk, ric, Rc), mat3T(Rc, RcT);
      mat3vec(Rk, tic, tmp);
      for (int c = 0; c < 3; c++) tc[c] = Pk[c] + tmp[c];
      for (int i = 0; i < n_landmarks; i++) {
        if ((rng() & 15) == 0) continue;  // a lost track
        const double dX[3] = {lm[3 * i] - tc[0], lm[3 * i + 1] - tc[1], lm[3 * i + 2] - tc[2]};
        double Xc[3];
        mat3vec(RcT, dX, Xc);
        if (Xc[2] < 0.5 || fabs(Xc[0]) > 0.9 * Xc[2] || fabs(Xc[1]) > 0.9 * Xc[2]) continue;
        VioObs o;
        o.id = i, o.x = Xc[0] / Xc[2] + uni(-1e-3, 1e-3), o.y = Xc[1] / Xc[2] + uni(-1e-3, 1e-3), o.z = 1.0;
        out.push_back(o);
      }
      for (size_t i = out.size(); i > 1; i--) std::swap(out[i - 1], out[rng() % i]);  // image_msg is not sorted
    };
    vio_features_create(W, &fms[s]);
    vio_features_t *fm = fms[s];
    std::vector<VioObs> ob;
    for (int fc = 0; fc < W; fc++) {  // the window fills on the host list
      observe(fc, ob);
      int enough = 0, pn = 0, tr = 0;
      if (vio_features_add_check_parallax(fm, fc, ob.data(), (int)ob.size(), &enough, &pn, &tr) != VIO_OK) msg.add("slot %d: fill failed", s);
    }
    SimStore &S = stores[s];
    {  // promotion: the list goes to the slot as it stands (bank 0)
      int n = 0, np = 0;
      vio_features_dump(fm, nullptr, 0, &n, nullptr, 0, &np);
      std::vector<VioFeatureInfo> info(n + 1);
      std::vector<double> pts(3 * (size_t)np + 3);
      vio_features_dump(fm, info.data(), n, &n, pts.data(), np, &np);
      if (n > Lcap) return -1;
      size_t p = 0;
      for (int i = 0; i < n; i++) {
        S.fid[0][i] = info[i].id, S.start[0][i] = info[i].start_frame, S.nobs[0][i] = info[i].n_obs, S.flag[0][i] = info[i].solve_flag;
        S.depth[0][i] = info[i].estimated_depth;
        for (int j = 0; j < info[i].n_obs; j++, p++)
          for (int c = 0; c < 3; c++) S.obs[0][((size_t)i * P + j) * 3 + c] = pts[3 * p + c];
      }
      S.ctl[st::C_N] = n, S.ctl[st::C_BANK] = 0;
    }
    Ps[s].resize(3 * P), Rs[s].resize(9 * P);
    for (int i = 0; i < P; i++) pose_at(i, &Ps[s][3 * i], &Rs[s][9 * i]);
    observe(W, ob);
    if ((int)ob.size() > Ocap) return -1;
    // ---- host list with the slot's camera
    int enough = 0, pn = 0, tr = 0;
    if (vio_features_add_check_parallax(fm, W, ob.data(), (int)ob.size(), &enough, &pn, &tr) != VIO_OK) msg.add("slot %d: host add failed", s);
    if (vio_features_triangulate(fm, Ps[s].data(), Rs[s].data(), tic, ric) != VIO_OK) msg.add("slot %d: host triangulate failed", s);
    // ---- store, pass 1, the way store_ingest_kernel runs slot s
    {
      st::Bank bk = S.bank(0);
      st::Lds l = S.lds();
      const st::SlotCamera cam = st::slot_camera(tic0, ric0, kRec, (s + shift) % kSlots);
      simt::launch(st::kThreads, [&](int tid) {
        st::Cx cx{tid, st::kThreads};
        st::store_ingest(cx, S.d, bk, S.ctl.data(), l, ob.data(), (int)ob.size(), Ps[s].data(), Rs[s].data(), cam.tic, cam.ric);
      }, order);
    }
    if (S.ctl[st::C_STATUS] != VIO_OK) msg.add("slot %d: store status %d", s, S.ctl[st::C_STATUS]);
    {
      int n = 0, np = 0;
      vio_features_dump(fm, nullptr, 0, &n, nullptr, 0, &np);
      std::vector<VioFeatureInfo> info(n + 1);
      std::vector<double> pts(3 * (size_t)np + 3);
      vio_features_dump(fm, info.data(), n, &n, pts.data(), np, &np);
      const int b = S.ctl[st::C_BANK];
      if (S.ctl[st::C_N] != n) msg.add("slot %d: list length %d, store %d", s, n, S.ctl[st::C_N]);
      long long solved = 0;
      for (int i = 0; i < n && S.ctl[st::C_N] == n && msg.fails < 20; i++) {
        if (S.fid[b][i] != info[i].id || S.start[b][i] != info[i].start_frame || S.nobs[b][i] != info[i].n_obs)
          msg.add("slot %d entry %d: id %d/%d start %d/%d nobs %d/%d", s, i, info[i].id, S.fid[b][i], info[i].start_frame, S.start[b][i],
                  info[i].n_obs, S.nobs[b][i]);
        if (memcmp(&S.depth[b][i], &info[i].estimated_depth, 8) != 0)
          msg.add("slot %d entry %d (id %d): depth %.17g, store %.17g", s, i, info[i].id, info[i].estimated_depth, S.depth[b][i]);
        solved += info[i].estimated_depth > 0 && info[i].estimated_depth != st::kInitDepth;
      }
      if (stats) stats[2 * s] = solved;
    }
  }
  // ---- pass 4, one job per slot in the caller's order, the way store_keyframe_kernel runs job j
  for (int j = 0; j < kSlots && msg.fails < 20; j++) {
    const int s = jobs[j];
    if (s < 0 || s >= kSlots) return -1;
    SimStore &S = stores[s];
    const double *c = cams + 16 * s;
    VioConfig cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.window_size = W, cfg.fx = c[0], cfg.fy = c[1], cfg.cx = c[2], cfg.cy = c[3];
    std::vector<int> want_ids(cap, -1), got_ids(cap, -1);
    std::vector<float> want_px(2 * cap, -1.f), want_norm(2 * cap, -1.f), got_px(2 * cap, std::numeric_limits<float>::quiet_NaN()),
        got_norm(2 * cap, std::numeric_limits<float>::quiet_NaN());
    std::vector<double> want_cloud(3 * cap, -1.0), got_cloud(3 * cap, kNan);
    int want_n = -1, got_n = -1;
    if (vio_features_keyframe(fms[s], &cfg, Ps[s].data(), Rs[s].data(), c + 4, c + 7, cap, want_ids.data(), want_px.data(), want_norm.data(),
                              want_cloud.data(), &want_n) != VIO_OK)
      msg.add("slot %d: host keyframe failed", s);
    const st::Bank bk = S.bank(S.ctl[st::C_BANK] & 1);
    std::vector<int> part(st::kThreads / 64 + 1, -1);
    const st::KeyOut o{got_ids.data(), got_px.data(), got_norm.data(), got_cloud.data(), &got_n, cap};
    const st::SlotCamera cam = st::slot_camera(tic0, ric0, kRec, (s + shift) % kSlots);
    const st::Intrinsics in = st::job_intrinsics(intr.data(), (j + shift) % kSlots, kNan, kNan, kNan, kNan);
    simt::launch(st::kThreads, [&](int tid) {
      st::Cx cx{tid, st::kThreads};
      st::store_keyframe(cx, S.d, bk, S.ctl.data(), part.data(), Ps[s].data(), Rs[s].data(), cam.tic, cam.ric, in.fx, in.fy, in.cx, in.cy, o);
    }, order);
    if (stats) stats[2 * s + 1] = want_n;
    if (got_n != want_n) {
      msg.add("job %d (slot %d): %d keyframe features, store %d", j, s, want_n, got_n);
      continue;
    }
    for (int k = 0; k < want_n && msg.fails < 20; k++) {
      if (got_ids[k] != want_ids[k]) msg.add("job %d (slot %d) feature %d: id %d, store %d", j, s, k, want_ids[k], got_ids[k]);
      if (memcmp(&got_px[2 * k], &want_px[2 * k], 8) != 0)
        msg.add("job %d (slot %d) feature %d: px %.9g %.9g, store %.9g %.9g", j, s, k, want_px[2 * k], want_px[2 * k + 1], got_px[2 * k], got_px[2 * k + 1]);
      if (memcmp(&got_norm[2 * k], &want_norm[2 * k], 8) != 0) msg.add("job %d (slot %d) feature %d: norm differs", j, s, k);
      if (memcmp(&got_cloud[3 * k], &want_cloud[3 * k], 24) != 0)
        msg.add("job %d (slot %d) feature %d: cloud %.17g %.17g %.17g, store %.17g %.17g %.17g", j, s, k, want_cloud[3 * k], want_cloud[3 * k + 1],
                want_cloud[3 * k + 2], got_cloud[3 * k], got_cloud[3 * k + 1], got_cloud[3 * k + 2]);
    }
  }
  for (vio_features_t *fm : fms)
    if (fm) vio_features_destroy(fm);
  return msg.fails;
}
