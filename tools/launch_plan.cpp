// Drives every entry point of the C ABI (include/mgacbam.h, include/mgaspade.h) over valid and invalid levels, linked against the
// recording stand-in for the HIP runtime (launch_plan_hip.cpp): the output is the library's launch plan -- per call its return code,
// message and launches.  Device pointers are made-up aligned addresses; the library never dereferences them.  argv[1]: workgroups per
// CU the stand-in's occupancy query answers (0: k_gate never eligible).  Only the public ABI is used, so one source serves any revision.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include <string>
#include "mgacbam.h"
#include "mgaspade.h"

extern "C" void stub_set_occupancy(int per_cu);
extern "C" void stub_fail_next_launch(void);

static void* const ST = reinterpret_cast<void*>(0x5151);
static char* dev(size_t bytes = 1 << 20) {   // a fresh 256-byte aligned "device" address
  static size_t next = size_t(1) << 32;
  char* p = reinterpret_cast<char*>(next);
  next += (bytes + 255) & ~size_t(255);
  return p;
}
static float* devf() { return reinterpret_cast<float*>(dev()); }
static int rc(const char* what, int code) { printf("%s -> %d %s\n", what, code, code ? mgacbam_last_error() : ""); return code; }
static const char* F(const char* fmt, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0, int g = 0, int h = 0, int i = 0, int j = 0, int k = 0, int l = 0) {
  static char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c, d, e, f, g, h, i, j, k, l);
  return buf;
}
struct Shape { int B, C, H, W; };
static const Shape kShapes[] = {{2, 64, 16, 16}, {2, 20, 10, 10}, {1, 6, 5, 7}, {4, 256, 40, 40}, {2, 24, 8, 12}, {3, 512, 20, 20}, {1, 260, 7, 9}};
static const int kDtypes[] = {MGACBAM_F32, MGACBAM_F16, MGACBAM_BF16};

// ---- MaskCBAM
static mgacbam_params_t cbam_params(int hidden, int k) { return {devf(), devf(), devf(), devf(), devf(), devf(), hidden, k, 1, 1e-4f, 1e-6f}; }
static mgacbam_fwd_level_t cbam_fwd(int dt, Shape s, int hid, int k, bool mask, int flags) {
  mgacbam_fwd_level_t L{};
  L.x = dev(); L.y = dev(); L.mask = mask ? devf() : nullptr; L.ctx = dev(); L.ctx_bytes = mgacbam_ctx_bytes(s.B, s.C, s.H, s.W, hid);
  L.p = cbam_params(hid, k); L.B = s.B; L.C = s.C; L.H = s.H; L.W = s.W; L.dtype = dt; L.flags = flags;
  L.ws = dev(); L.ws_bytes = mgacbam_fwd_ws_bytes(s.B, s.C, s.H, s.W, hid, flags);
  return L;
}
static mgacbam_bwd_level_t cbam_bwd(int dt, Shape s, int hid, int k, bool mask, bool gmask, int flags) {
  mgacbam_bwd_level_t L{};
  L.x = dev(); L.gy = dev(); L.gx = dev(); L.mask = mask ? devf() : nullptr; L.gmask = gmask ? devf() : nullptr;
  L.ctx = dev(); L.ctx_bytes = mgacbam_ctx_bytes(s.B, s.C, s.H, s.W, hid);
  L.scratch = dev(); L.scratch_bytes = mgacbam_bwd_scratch_bytes_flags(s.B, s.C, s.H, s.W, hid, k, flags);
  L.gw1 = devf(); L.gb1 = devf(); L.gw2 = devf(); L.gb2 = devf(); L.gwsa = devf(); L.gbeta = devf();
  L.p = cbam_params(hid, k); L.B = s.B; L.C = s.C; L.H = s.H; L.W = s.W; L.dtype = dt; L.flags = flags;
  return L;
}
static const int kFwdStages[] = {MGACBAM_FWD_POOL, MGACBAM_FWD_CHAN, MGACBAM_FWD_APPLY, MGACBAM_FWD_POOL | MGACBAM_FWD_CHAN, MGACBAM_FWD_ALL,
                                 MGACBAM_FWD_ALL | MGACBAM_FWD_FUSE, MGACBAM_FWD_CHAN | MGACBAM_FWD_APPLY | MGACBAM_FWD_FUSE};
static const int kBwdStages[] = {
    MGACBAM_BWD_REDUCE1, MGACBAM_BWD_CONVT, MGACBAM_BWD_REDUCE2, MGACBAM_BWD_WSA, MGACBAM_BWD_PARAMGRAD, MGACBAM_BWD_APPLY, MGACBAM_BWD_PARAMS,
    MGACBAM_BWD_FUSE | MGACBAM_BWD_REDUCE2 | MGACBAM_BWD_WSA, MGACBAM_BWD_FUSE | MGACBAM_BWD_PARAMGRAD | MGACBAM_BWD_APPLY, MGACBAM_BWD_ALL,
    MGACBAM_BWD_ALL | MGACBAM_BWD_FOLD, MGACBAM_BWD_FOLD | MGACBAM_BWD_REDUCE1 | MGACBAM_BWD_CONVT,
    MGACBAM_BWD_FOLD | (MGACBAM_BWD_ALL & ~MGACBAM_BWD_FUSE)};
static void cbam(bool full) {
  for (int dt : kDtypes) for (Shape s : kShapes) for (int nhwc = 0; nhwc < 2; ++nhwc) for (int mask = 0; mask < 2; ++mask)
    for (int k : {1, 3, 5, 7, 9}) for (int hid : {2, 4, 8, 32}) {
      if (!full && (k == 1 || k == 9 || hid == 8 || s.C == 24)) continue;
      for (int proj = 0; proj < 2; ++proj) {
        const mgacbam_fwd_level_t L = cbam_fwd(dt, s, hid, k, mask, (nhwc ? MGACBAM_LAYOUT_NHWC : 0) | (proj ? MGACBAM_FWD_SAVE_PROJ : 0));
        for (int st : kFwdStages)
          rc(F("cbam fwd dt=%d B=%d C=%d H=%d W=%d nhwc=%d mask=%d k=%d hid=%d proj=%d stages=%d", dt, s.B, s.C, s.H, s.W, nhwc, mask, k, hid, proj, st),
             mgacbam_forward_stages(&L, 1, st, ST));
        for (int gm = 0; gm <= mask; ++gm) {
          const mgacbam_bwd_level_t Lb = cbam_bwd(dt, s, hid, k, mask, gm, (nhwc ? MGACBAM_LAYOUT_NHWC : 0) | (proj ? MGACBAM_BWD_HAVE_PROJ : 0));
          for (int st : kBwdStages)
            rc(F("cbam bwd dt=%d B=%d C=%d H=%d W=%d nhwc=%d mask=%d gmask=%d k=%d hid=%d have=%d stages=%d", dt, s.B, s.C, s.H, s.W, nhwc, mask, gm, k, hid, proj, st),
               mgacbam_backward_stages(&Lb, 1, st, ST));
        }
      }
    }
  // pyramids of MGACBAM_MAX_LEVELS levels with mixed signatures: the grouping, its order and the group size limit
  mgacbam_fwd_level_t P[MGACBAM_MAX_LEVELS];
  mgacbam_bwd_level_t Q[MGACBAM_MAX_LEVELS];
  for (int v = 0; v < 4; ++v) {
    for (int l = 0; l < MGACBAM_MAX_LEVELS; ++l) {
      const Shape s = v == 3 ? Shape{2, 64 << (l % 3), 32 >> (l % 3), 32 >> (l % 3)} : kShapes[(l * (v + 1)) % 6];
      const int dt = v == 3 ? 0 : kDtypes[(l / (v + 1)) % 3], nhwc = v == 0 ? 0 : v == 3 ? l / 6 : l & 1, k = v == 2 ? 3 + 2 * (l % 3) : 7;
      P[l] = cbam_fwd(dt, s, 4, k, l != 5, nhwc ? MGACBAM_LAYOUT_NHWC : 0);
      Q[l] = cbam_bwd(dt, s, 4, k, l != 5, l != 5 && l != 2, nhwc ? MGACBAM_LAYOUT_NHWC : 0);
    }
    for (int n : {3, 5, MGACBAM_MAX_LEVELS}) {
      rc(F("cbam fwd pyramid v=%d n=%d", v, n), mgacbam_forward(P, n, ST));
      rc(F("cbam fwd pyramid fused v=%d n=%d", v, n), mgacbam_forward_stages(P, n, MGACBAM_FWD_ALL | MGACBAM_FWD_FUSE, ST));
      rc(F("cbam bwd pyramid v=%d n=%d", v, n), mgacbam_backward(Q, n, ST));
      rc(F("cbam bwd pyramid folded v=%d n=%d", v, n), mgacbam_backward_stages(Q, n, MGACBAM_BWD_ALL | MGACBAM_BWD_FOLD, ST));
    }
  }
}
// ---- MaskECA
static void eca(bool full) {
  for (int dt : kDtypes) for (Shape s : kShapes) for (int nhwc = 0; nhwc < 2; ++nhwc) for (int mask = 0; mask < 2; ++mask) for (int k : {3, 5}) {
    if (!full && k == 5) continue;
    const int fl = nhwc ? MGACBAM_LAYOUT_NHWC : 0;
    mgacbam_eca_fwd_level_t L{};
    L.x = dev(); L.y = dev(); L.mask = mask ? devf() : nullptr; L.ctx = dev(); L.ctx_bytes = mgacbam_eca_ctx_bytes_flags(s.B, s.C, s.H, s.W, fl);
    L.p = {devf(), devf(), k, 1, 1e-4f, 1e-6f}; L.B = s.B; L.C = s.C; L.H = s.H; L.W = s.W; L.dtype = dt; L.flags = fl;
    rc(F("eca fwd dt=%d B=%d C=%d H=%d W=%d nhwc=%d mask=%d k=%d", dt, s.B, s.C, s.H, s.W, nhwc, mask, k), mgacbam_eca_forward(&L, 1, ST));
    for (int gm = 0; gm <= mask; ++gm) {
      mgacbam_eca_bwd_level_t Lb{};
      Lb.x = dev(); Lb.gy = dev(); Lb.gx = dev(); Lb.mask = L.mask; Lb.gmask = gm ? devf() : nullptr; Lb.ctx = L.ctx; Lb.ctx_bytes = L.ctx_bytes;
      Lb.scratch = dev(); Lb.scratch_bytes = mgacbam_eca_scratch_bytes_flags(s.B, s.C, s.H, s.W, fl); Lb.gw = devf(); Lb.gbeta = devf();
      Lb.p = L.p; Lb.B = s.B; Lb.C = s.C; Lb.H = s.H; Lb.W = s.W; Lb.dtype = dt; Lb.flags = fl;
      rc(F("eca bwd dt=%d B=%d C=%d H=%d W=%d nhwc=%d mask=%d gmask=%d k=%d", dt, s.B, s.C, s.H, s.W, nhwc, mask, gm, k), mgacbam_eca_backward(&Lb, 1, ST));
      if (s.C == 64 && mask && gm) {   // a pyramid: the same level in both layouts and two element types, twice over
        mgacbam_eca_fwd_level_t P[MGACBAM_MAX_LEVELS];
        mgacbam_eca_bwd_level_t Q[MGACBAM_MAX_LEVELS];
        for (int l = 0; l < MGACBAM_MAX_LEVELS; ++l) {
          P[l] = L; Q[l] = Lb;
          P[l].flags = Q[l].flags = (l & 1) ? MGACBAM_LAYOUT_NHWC : 0; P[l].dtype = Q[l].dtype = (l & 2) ? MGACBAM_F32 : dt;
          P[l].C = Q[l].C = 64 - 8 * (l / 4);
        }
        rc(F("eca fwd pyramid dt=%d", dt), mgacbam_eca_forward(P, MGACBAM_MAX_LEVELS, ST));
        rc(F("eca bwd pyramid dt=%d", dt), mgacbam_eca_backward(Q, MGACBAM_MAX_LEVELS, ST));
      }
    }
  }
}
// ---- MGAMaskHead
static mgahead_bwd_level_t head_level(int dt, Shape s, int hid, int flags, mgahead_fwd_level_t& Lf) {
  Lf = mgahead_fwd_level_t{};
  Lf.x = dev(); Lf.logits = dev(); Lf.ctx = dev(); Lf.ctx_bytes = mgahead_ctx_bytes_flags(s.B, s.C, s.H, s.W, hid, flags);
  Lf.p = {devf(), devf(), devf(), devf(), devf(), reinterpret_cast<int64_t*>(dev()), devf(), devf(), hid, 1e-3f, 0.03f, 1};
  Lf.B = s.B; Lf.C = s.C; Lf.H = s.H; Lf.W = s.W; Lf.dtype = dt; Lf.flags = flags & ~MGAHEAD_BWD_ACCUM_GX;
  mgahead_bwd_level_t L{};
  L.x = Lf.x; L.g_logits = dev(); L.g_logits2 = (flags & MGAHEAD_BWD_ACCUM_GX) ? devf() : nullptr; L.ctx = Lf.ctx; L.ctx_bytes = Lf.ctx_bytes;
  L.scratch = dev(); L.scratch_bytes = mgahead_bwd_scratch_bytes_flags(s.B, s.C, s.H, s.W, hid, flags); L.gx = dev();
  L.gw1 = devf(); L.gbn_weight = devf(); L.gbn_bias = devf(); L.gwh = devf(); L.gbh = devf();
  L.p = Lf.p; L.B = s.B; L.C = s.C; L.H = s.H; L.W = s.W; L.dtype = dt; L.flags = flags;
  return L;
}
static void head() {
  mgahead_fwd_level_t P[MGACBAM_MAX_LEVELS];
  mgahead_bwd_level_t Q[MGACBAM_MAX_LEVELS];
  for (int dt : kDtypes) for (int accum : {0, int(MGAHEAD_BWD_ACCUM_GX)}) for (int lf32 : {0, int(MGAHEAD_LOGITS_F32)}) for (int cl : {0, int(MGAHEAD_LAYOUT_NHWC)}) {
    const int flags = accum | lf32 | cl;
    int n = 0;
    for (Shape s : kShapes) for (int hid : {16, 20, 64, 160}) {
      mgahead_fwd_level_t Lf;
      const mgahead_bwd_level_t L = head_level(dt, s, hid, flags, Lf);
      rc(F("head fwd dt=%d B=%d C=%d H=%d W=%d hid=%d flags=%d", dt, s.B, s.C, s.H, s.W, hid, flags), mgahead_forward(&Lf, 1, ST));
      rc(F("head bwd dt=%d B=%d C=%d H=%d W=%d hid=%d flags=%d", dt, s.B, s.C, s.H, s.W, hid, flags), mgahead_backward(&L, 1, ST));
      if (hid != 20 && (n < MGACBAM_MAX_LEVELS) && (s.C == 64 || s.C == 256 || s.C == 512)) { P[n] = Lf; Q[n++] = L; }
    }
    for (int l = 0; l < n; ++l) if (l % 3 == 2) { P[l].flags ^= MGAHEAD_LAYOUT_NHWC; Q[l].flags ^= MGAHEAD_LAYOUT_NHWC;   // mixed layouts: sizes follow
      P[l].ctx_bytes = Q[l].ctx_bytes = mgahead_ctx_bytes_flags(P[l].B, P[l].C, P[l].H, P[l].W, P[l].p.hidden, P[l].flags);
      Q[l].scratch_bytes = mgahead_bwd_scratch_bytes_flags(P[l].B, P[l].C, P[l].H, P[l].W, P[l].p.hidden, P[l].flags); }
    rc(F("head fwd pyramid dt=%d flags=%d n=%d", dt, flags, n), mgahead_forward(P, n, ST));
    rc(F("head bwd pyramid dt=%d flags=%d n=%d", dt, flags, n), mgahead_backward(Q, n, ST));
  }
}
// ---- MaskSPADE
static const int kSpadeNhwc = 2;   // MGASPADE_LAYOUT_NHWC, as a literal: the driver also builds against a revision from before the flag (which refuses it)
static mgaspade_level_t spade_level(int dt, Shape s, int hid, int bn, int train, bool mask, bool gmask, int save, int flags = 0) {
  mgaspade_level_t L{};
  L.x = dev(); L.y = dev(); L.gy = dev(); L.gx = dev(); L.mask = mask ? devf() : nullptr; L.gmask = gmask ? devf() : nullptr;
  L.w0 = devf(); L.b0 = devf(); L.wg = devf(); L.bg = devf(); L.wb = devf(); L.bb = devf();
  L.running_mean = devf(); L.running_var = devf(); L.num_batches_tracked = reinterpret_cast<long long*>(dev());
  L.gw0 = devf(); L.gb0 = devf(); L.gwg = devf(); L.gbg = devf(); L.gwb = devf(); L.gbb = devf();
  L.ctx = dev(); L.ctx_bytes = mgaspade_ctx_bytes(s.B, s.C, s.H, s.W, hid); L.scratch = dev(); L.scratch_bytes = mgaspade_scratch_bytes(s.B, s.C, s.H, s.W, hid);
  L.B = s.B; L.C = s.C; L.H = s.H; L.W = s.W; L.hidden = hid; L.dtype = dt; L.norm_type = bn; L.training = train; L.use_sigmoid_mask = 1;
  L.save_gamma = save; L.eps = 1e-5f; L.momentum = 0.1f; L.flags = flags;
  return L;
}
static void spade() {
  mgaspade_level_t P[MGACBAM_MAX_LEVELS];
  for (int dt : kDtypes) {
    int n = 0;
    for (Shape s : {Shape{2, 64, 16, 16}, Shape{2, 16, 10, 10}, Shape{1, 48, 5, 7}, Shape{2, 256, 40, 40}, Shape{1, 1024, 33, 20}})
      for (int hid : {16, 128}) for (int norm = 0; norm < 3; ++norm) for (int mask = 0; mask < 2; ++mask) for (int gs = 0; gs <= mask; ++gs) {
        const mgaspade_level_t L = spade_level(dt, s, hid, norm != 0, norm == 2, mask, gs, gs);
        rc(F("spade fwd dt=%d B=%d C=%d H=%d W=%d hid=%d norm=%d mask=%d save=%d", dt, s.B, s.C, s.H, s.W, hid, norm, mask, gs), mgaspade_forward(&L, 1, ST));
        rc(F("spade bwd dt=%d B=%d C=%d H=%d W=%d hid=%d norm=%d mask=%d gmask=%d", dt, s.B, s.C, s.H, s.W, hid, norm, mask, gs), mgaspade_backward(&L, 1, ST));
        if (n < MGACBAM_MAX_LEVELS && hid == 16 && (norm + mask + gs) % 2) P[n++] = L;
        if (hid != 16) continue;
        const mgaspade_level_t N = spade_level(dt, s, hid, norm != 0, norm == 2, mask, gs, gs, kSpadeNhwc);
        rc(F("spade fwd nhwc dt=%d B=%d C=%d H=%d W=%d hid=%d norm=%d mask=%d save=%d", dt, s.B, s.C, s.H, s.W, hid, norm, mask, gs), mgaspade_forward(&N, 1, ST));
        rc(F("spade bwd nhwc dt=%d B=%d C=%d H=%d W=%d hid=%d norm=%d mask=%d gmask=%d", dt, s.B, s.C, s.H, s.W, hid, norm, mask, gs), mgaspade_backward(&N, 1, ST));
      }
    rc(F("spade fwd pyramid dt=%d n=%d", dt, n), mgaspade_forward(P, n, ST));
    rc(F("spade bwd pyramid dt=%d n=%d", dt, n), mgaspade_backward(P, n, ST));
    for (int l = 0; l < n; l += 2) P[l].flags = kSpadeNhwc;   // levels of both layouts in one call: the sizes do not change
    rc(F("spade fwd pyramid mixed layouts dt=%d n=%d", dt, n), mgaspade_forward(P, n, ST));
    rc(F("spade bwd pyramid mixed layouts dt=%d n=%d", dt, n), mgaspade_backward(P, n, ST));
  }
}
// ---- calls of three and five small levels for the four level families: what decides the launch groups, mixed within one call
// pattern 0 / 1: layouts alternate (NCHW first / channels-last first), mask, dL/dmask (gamma kept) and element type vary from level to level;
// pattern 2 / 3: a block of one layout, then the other (channels-last first / NCHW first), fp32, two shapes of one vector width, so groups hold
// several levels and their order inside a group shows; pattern 4 / 5: ONE signature throughout (NCHW / channels-last): five levels exceed a group
struct Mix { Shape s; int dt, nhwc, mask, gmask, keep; };
static Mix mix_level(int pattern, int l, int n, bool spade) {
  static const Shape any[] = {{2, 64, 16, 16}, {2, 20, 10, 10}, {1, 6, 5, 7}, {1, 260, 7, 9}};
  static const Shape sp[] = {{2, 64, 16, 16}, {2, 32, 10, 10}, {1, 16, 5, 7}, {1, 256, 7, 9}};   // MaskSPADE takes C % 16 == 0
  const Shape* S = spade ? sp : any;
  Mix m;
  if (pattern < 2) {
    m.s = S[l % 4]; m.dt = (l / 2) % 2 ? MGACBAM_F16 : MGACBAM_F32; m.nhwc = (l + pattern) & 1; m.mask = l % 3 != 1; m.gmask = m.mask && l != 3;
    m.keep = l % 2 == 0;
  } else if (pattern < 4) {
    m.s = S[l % 2]; m.dt = MGACBAM_F32; m.nhwc = (pattern == 2) == (l < n / 2); m.mask = 1; m.gmask = l != 1; m.keep = l != 2;
  } else {
    m.s = S[l % 2]; m.dt = MGACBAM_F32; m.nhwc = pattern - 4; m.mask = 1; m.gmask = 1; m.keep = 1;
  }
  return m;
}
static void mixed() {
  for (int pattern = 0; pattern < 6; ++pattern) for (int n : {3, 5}) {
    mgacbam_fwd_level_t CF[5]; mgacbam_bwd_level_t CB[5];
    mgacbam_eca_fwd_level_t EF[5]; mgacbam_eca_bwd_level_t EB[5];
    mgahead_fwd_level_t HF[5]; mgahead_bwd_level_t HB[5];
    mgaspade_level_t SF[5], SB[5];
    for (int l = 0; l < n; ++l) {
      const Mix m = mix_level(pattern, l, n, false);
      const Shape s = m.s;
      const int fl = m.nhwc ? MGACBAM_LAYOUT_NHWC : 0;
      CF[l] = cbam_fwd(m.dt, s, 4, 7, m.mask, fl);
      CB[l] = cbam_bwd(m.dt, s, 4, 7, m.mask, m.gmask, fl);
      mgacbam_eca_fwd_level_t& L = EF[l];
      L = mgacbam_eca_fwd_level_t{};
      L.x = dev(); L.y = dev(); L.mask = m.mask ? devf() : nullptr; L.ctx = dev(); L.ctx_bytes = mgacbam_eca_ctx_bytes_flags(s.B, s.C, s.H, s.W, fl);
      L.p = {devf(), devf(), 3, 1, 1e-4f, 1e-6f}; L.B = s.B; L.C = s.C; L.H = s.H; L.W = s.W; L.dtype = m.dt; L.flags = fl;
      mgacbam_eca_bwd_level_t& Lb = EB[l];
      Lb = mgacbam_eca_bwd_level_t{};
      Lb.x = dev(); Lb.gy = dev(); Lb.gx = dev(); Lb.mask = L.mask; Lb.gmask = m.gmask ? devf() : nullptr; Lb.ctx = L.ctx; Lb.ctx_bytes = L.ctx_bytes;
      Lb.scratch = dev(); Lb.scratch_bytes = mgacbam_eca_scratch_bytes_flags(s.B, s.C, s.H, s.W, fl); Lb.gw = devf(); Lb.gbeta = devf();
      Lb.p = L.p; Lb.B = s.B; Lb.C = s.C; Lb.H = s.H; Lb.W = s.W; Lb.dtype = m.dt; Lb.flags = fl;
      HB[l] = head_level(m.dt, s, 16, (m.nhwc ? MGAHEAD_LAYOUT_NHWC : 0) | (m.keep ? 0 : MGAHEAD_LOGITS_F32), HF[l]);
      const Mix ms = mix_level(pattern, l, n, true);
      SF[l] = spade_level(ms.dt, ms.s, 16, l % 2, 1, ms.mask, false, ms.mask && ms.keep, ms.nhwc ? kSpadeNhwc : 0);
      SB[l] = spade_level(ms.dt, ms.s, 16, l % 2, 1, ms.mask, ms.gmask, 1, ms.nhwc ? kSpadeNhwc : 0);
    }
    rc(F("mixed cbam fwd pattern=%d n=%d", pattern, n), mgacbam_forward(CF, n, ST));
    rc(F("mixed cbam fwd fused pattern=%d n=%d", pattern, n), mgacbam_forward_stages(CF, n, MGACBAM_FWD_ALL | MGACBAM_FWD_FUSE, ST));
    rc(F("mixed cbam bwd pattern=%d n=%d", pattern, n), mgacbam_backward(CB, n, ST));
    rc(F("mixed cbam bwd folded pattern=%d n=%d", pattern, n), mgacbam_backward_stages(CB, n, MGACBAM_BWD_ALL | MGACBAM_BWD_FOLD, ST));
    rc(F("mixed eca fwd pattern=%d n=%d", pattern, n), mgacbam_eca_forward(EF, n, ST));
    rc(F("mixed eca bwd pattern=%d n=%d", pattern, n), mgacbam_eca_backward(EB, n, ST));
    rc(F("mixed head fwd pattern=%d n=%d", pattern, n), mgahead_forward(HF, n, ST));
    rc(F("mixed head bwd pattern=%d n=%d", pattern, n), mgahead_backward(HB, n, ST));
    rc(F("mixed spade fwd pattern=%d n=%d", pattern, n), mgaspade_forward(SF, n, ST));
    rc(F("mixed spade bwd pattern=%d n=%d", pattern, n), mgaspade_backward(SB, n, ST));
  }
}
// ---- segmentation loss, Kendall combine, gater, resize
static void loss_side() {
  const mgaseg_cfg_t cfg{1.f, 1.f, 1.f, 0.5f, 0, 0.5f, 0.6f, 0.5f};
  const mgapmg_cfg_t pc{0.5f, 0.05f, 0.5f, 1}, bad_tau{0.f, 0.05f, 0.5f, 1};
  for (int dt = 0; dt < 4; ++dt) for (int n = 0; n <= MGASEG_MAX_LEVELS + 1; ++n) {
    mgaseg_level_t L[MGASEG_MAX_LEVELS + 1];
    for (int l = 0; l <= MGASEG_MAX_LEVELS; ++l) L[l] = {dev(), devf(), dev(), 2 + l, 80 >> l, 80 >> l, 160, 160, dt, 1.f, l & 1};
    const size_t ws = mgaseg_ws_bytes(L, n);
    printf("segloss dt=%d n=%d ws=%zu\n", dt, n, ws);
    rc("seg fwd", mgaseg_forward(L, n, &cfg, dev(), ws, devf(), ST));
    rc("seg bwd", mgaseg_backward(L, n, &cfg, dev(), ws, devf(), ST));
    rc("seg kendall fwd", mgaseg_kendall_forward(L, n, &cfg, dev(), ws, devf(), devf(), 3, devf(), devf(), ST));
    rc("seg kendall bwd", mgaseg_kendall_backward(L, n, &cfg, dev(), ws, devf(), devf(), 3, devf(), devf(), devf(), devf(), devf(), ST));
    if (n == 2) {
      rc("seg fwd short ws", mgaseg_forward(L, n, &cfg, dev(), ws - 16, devf(), ST));
      rc("seg bwd NULL gout", mgaseg_backward(L, n, &cfg, dev(), ws, nullptr, ST));
      rc("seg kendall fwd n_det", mgaseg_kendall_forward(L, n, &cfg, dev(), ws, devf(), devf(), 5000, devf(), devf(), ST));
      L[1].dtype = (dt + 1) % 3; rc("seg fwd mixed dtype", mgaseg_forward(L, n, &cfg, dev(), ws, devf(), ST));
      L[1].dtype = dt; L[1].resize = 2; rc("seg fwd resize mode", mgaseg_forward(L, n, &cfg, dev(), ws, devf(), ST));
      L[1].resize = 0; L[1].target = nullptr; L[0].H = 0; rc("seg bwd two faults", mgaseg_backward(L, n, &cfg, dev(), ws, devf(), ST));
    }
  }
  for (int nd : {0, 1, 4096, 4097}) {
    rc(F("kendall fwd n_det=%d", nd), mgakendall_forward(devf(), nd, devf(), devf(), devf(), ST));
    rc(F("kendall bwd n_det=%d", nd), mgakendall_backward(devf(), nd, devf(), devf(), devf(), devf(), devf(), devf(), ST));
  }
  rc("kendall fwd NULL", mgakendall_forward(devf(), 3, nullptr, devf(), devf(), ST));
  for (size_t n : {size_t(0), size_t(1), size_t(1000), size_t(1) << 24}) {
    rc(F("gater fwd n=%d", int(n)), mgapmg_forward(devf(), devf(), devf(), devf(), devf(), n, &pc, ST));
    rc(F("gater bwd n=%d", int(n)), mgapmg_backward(devf(), devf(), devf(), devf(), n, &pc, ST));
  }
  rc("gater fwd tau", mgapmg_forward(devf(), devf(), devf(), devf(), devf(), 8, &bad_tau, ST));
  rc("gater bwd NULL cfg", mgapmg_backward(devf(), devf(), devf(), devf(), 8, nullptr, ST));
  rc("resize", mgacbam_resize_nearest(devf(), devf(), 6, 160, 160, 20, 20, ST));
  rc("resize large", mgacbam_resize_nearest(devf(), devf(), 64, 20, 20, 320, 320, ST));
  rc("resize bad", mgacbam_resize_nearest(devf(), devf(), 6, 0, 160, 20, 20, ST));
  rc("resize NULL", mgacbam_resize_nearest(nullptr, devf(), 6, 160, 160, 20, 20, ST));
}
// ---- invalid levels: `edit` spoils a copy of a valid level, `call` runs the entry point on it
template <typename Level, typename Call, typename Edit>
static void bad1(const char* entry, const char* fault, const Level& good, Call call, Edit edit) {
  Level L[2] = {good, good};
  edit(L[1]);
  rc(F((std::string(entry) + ": " + fault).c_str()), call(L, 2));
}
template <typename Level, typename Call>
static void bad(const char* entry, const Level& good, Call call) {
  rc(F((std::string(entry) + ": valid").c_str()), call(&good, 1));
  rc(F((std::string(entry) + ": levels NULL").c_str()), call(static_cast<const Level*>(nullptr), 1));
  Level many[MGACBAM_MAX_LEVELS + 1];
  for (Level& l : many) l = good;
  for (int n : {0, -1, MGACBAM_MAX_LEVELS + 1}) rc(F((std::string(entry) + ": n_levels=%d").c_str(), n), call(many, n));
  bad1(entry, "x NULL", good, call, [](Level& L) { L.x = nullptr; });
  bad1(entry, "ctx NULL", good, call, [](Level& L) { L.ctx = nullptr; });
  for (int dt : {-1, 3, 7}) bad1(entry, "dtype out of range", good, call, [&](Level& L) { L.dtype = dt; });
  bad1(entry, "x misaligned", good, call, [](Level& L) { L.x = static_cast<const char*>(L.x) + 2; });
  bad1(entry, "ctx misaligned", good, call, [](Level& L) { L.ctx = static_cast<char*>(const_cast<void*>(static_cast<const void*>(L.ctx))) + 4; });
  bad1(entry, "ctx short", good, call, [](Level& L) { L.ctx_bytes -= 16; });
  bad1(entry, "ctx empty", good, call, [](Level& L) { L.ctx_bytes = 0; });
  bad1(entry, "unknown flag bits", good, call, [](Level& L) { L.flags |= 0x4000; });
  bad1(entry, "C=0", good, call, [](Level& L) { L.C = 0; });
  bad1(entry, "C=70000", good, call, [](Level& L) { L.C = 70000; });
  bad1(entry, "C=40", good, call, [](Level& L) { L.C = 40; });   // (a shape the buffers were not sized for)
  bad1(entry, "W=600", good, call, [](Level& L) { L.W = 600; });
  bad1(entry, "H=-1", good, call, [](Level& L) { L.H = -1; });
  bad1(entry, "dtype and ctx short", good, call, [](Level& L) { L.dtype = 9; L.ctx_bytes = 8; });
  bad1(entry, "x misaligned and ctx short", good, call, [](Level& L) { L.x = static_cast<const char*>(L.x) + 2; L.ctx_bytes = 8; });
  bad1(entry, "x NULL and C=0", good, call, [](Level& L) { L.x = nullptr; L.C = 0; });
}
template <typename Level, typename Call>
static void bad_bwd(const char* entry, const Level& good, Call call) {   // what only the backward levels have
  bad1(entry, "scratch NULL", good, call, [](Level& L) { L.scratch = nullptr; });
  bad1(entry, "gx NULL", good, call, [](Level& L) { L.gx = nullptr; });
  bad1(entry, "scratch misaligned", good, call, [](Level& L) { L.scratch = static_cast<char*>(L.scratch) + 8; });
  bad1(entry, "gx misaligned", good, call, [](Level& L) { L.gx = static_cast<char*>(L.gx) + 2; });
  bad1(entry, "scratch short", good, call, [](Level& L) { L.scratch_bytes -= 16; });
  bad1(entry, "scratch short and ctx short", good, call, [](Level& L) { L.scratch_bytes = 16; L.ctx_bytes = 16; });
  bad1(entry, "gx misaligned and scratch short", good, call, [](Level& L) { L.gx = static_cast<char*>(L.gx) + 2; L.scratch_bytes = 16; });
}
static void invalid() {
  const Shape s{2, 64, 16, 16};
  for (int dt : {MGACBAM_F32, MGACBAM_BF16}) for (int nhwc = 0; nhwc < 2; ++nhwc) {
    const int fl = nhwc ? MGACBAM_LAYOUT_NHWC : 0;
    printf("invalid levels dt=%d nhwc=%d\n", dt, nhwc);
    const mgacbam_fwd_level_t cf = cbam_fwd(dt, s, 4, 7, true, fl);
    auto cfwd = [](const mgacbam_fwd_level_t* L, int n) { return mgacbam_forward(L, n, ST); };
    bad("mgacbam_forward", cf, cfwd);
    bad1("mgacbam_forward", "w1 NULL", cf, cfwd, [](mgacbam_fwd_level_t& L) { L.p.w1 = nullptr; });
    for (int k : {0, 4, 17}) bad1("mgacbam_forward", "bad k", cf, cfwd, [&](mgacbam_fwd_level_t& L) { L.p.k = k; });
    bad1("mgacbam_forward", "hidden=0", cf, cfwd, [](mgacbam_fwd_level_t& L) { L.p.hidden = 0; });
    bad1("mgacbam_forward", "ws NULL", cf, cfwd, [](mgacbam_fwd_level_t& L) { L.ws = nullptr; });
    bad1("mgacbam_forward", "ws short", cf, cfwd, [](mgacbam_fwd_level_t& L) { L.ws_bytes = 16; });
    bad1("mgacbam_forward", "mask misaligned", cf, cfwd, [](mgacbam_fwd_level_t& L) { L.mask += 1; });
    const mgacbam_bwd_level_t cb = cbam_bwd(dt, s, 4, 7, true, true, fl);
    auto cbwd = [](const mgacbam_bwd_level_t* L, int n) { return mgacbam_backward(L, n, ST); };
    bad("mgacbam_backward", cb, cbwd); bad_bwd("mgacbam_backward", cb, cbwd);
    bad1("mgacbam_backward", "gw2 NULL", cb, cbwd, [](mgacbam_bwd_level_t& L) { L.gw2 = nullptr; });
    bad1("mgacbam_backward", "gmask without mask", cb, cbwd, [](mgacbam_bwd_level_t& L) { L.mask = nullptr; });
    bad1("mgacbam_backward", "gmask misaligned", cb, cbwd, [](mgacbam_bwd_level_t& L) { L.gmask += 1; });
    mgacbam_eca_fwd_level_t ef{};
    ef.x = dev(); ef.y = dev(); ef.mask = devf(); ef.ctx = dev(); ef.ctx_bytes = mgacbam_eca_ctx_bytes_flags(s.B, s.C, s.H, s.W, fl);
    ef.p = {devf(), devf(), 3, 1, 1e-4f, 1e-6f}; ef.B = s.B; ef.C = s.C; ef.H = s.H; ef.W = s.W; ef.dtype = dt; ef.flags = fl;
    auto efwd = [](const mgacbam_eca_fwd_level_t* L, int n) { return mgacbam_eca_forward(L, n, ST); };
    bad("mgacbam_eca_forward", ef, efwd);
    bad1("mgacbam_eca_forward", "w NULL", ef, efwd, [](mgacbam_eca_fwd_level_t& L) { L.p.w = nullptr; });
    bad1("mgacbam_eca_forward", "k=4", ef, efwd, [](mgacbam_eca_fwd_level_t& L) { L.p.k = 4; });
    bad1("mgacbam_eca_forward", "C=4100", ef, efwd, [](mgacbam_eca_fwd_level_t& L) { L.C = 4100; });
    bad1("mgacbam_eca_forward", "mask misaligned", ef, efwd, [](mgacbam_eca_fwd_level_t& L) { L.mask += 1; });
    mgacbam_eca_bwd_level_t eb{};
    eb.x = dev(); eb.gy = dev(); eb.gx = dev(); eb.mask = devf(); eb.gmask = devf(); eb.ctx = ef.ctx; eb.ctx_bytes = ef.ctx_bytes; eb.scratch = dev();
    eb.scratch_bytes = mgacbam_eca_scratch_bytes_flags(s.B, s.C, s.H, s.W, fl); eb.gw = devf(); eb.gbeta = devf();
    eb.p = ef.p; eb.B = s.B; eb.C = s.C; eb.H = s.H; eb.W = s.W; eb.dtype = dt; eb.flags = fl;
    auto ebwd = [](const mgacbam_eca_bwd_level_t* L, int n) { return mgacbam_eca_backward(L, n, ST); };
    bad("mgacbam_eca_backward", eb, ebwd); bad_bwd("mgacbam_eca_backward", eb, ebwd);
    bad1("mgacbam_eca_backward", "gmask without mask", eb, ebwd, [](mgacbam_eca_bwd_level_t& L) { L.mask = nullptr; });
    bad1("mgacbam_eca_backward", "C=4100", eb, ebwd, [](mgacbam_eca_bwd_level_t& L) { L.C = 4100; });
    mgahead_fwd_level_t hf;
    const mgahead_bwd_level_t hb = head_level(dt, s, 16, nhwc ? MGAHEAD_LAYOUT_NHWC : 0, hf);
    auto hfwd = [](const mgahead_fwd_level_t* L, int n) { return mgahead_forward(L, n, ST); };
    auto hbwd = [](const mgahead_bwd_level_t* L, int n) { return mgahead_backward(L, n, ST); };
    bad("mgahead_forward", hf, hfwd);
    bad1("mgahead_forward", "logits NULL", hf, hfwd, [](mgahead_fwd_level_t& L) { L.logits = nullptr; });
    bad1("mgahead_forward", "wh NULL", hf, hfwd, [](mgahead_fwd_level_t& L) { L.p.wh = nullptr; });
    bad1("mgahead_forward", "hidden=2000", hf, hfwd, [](mgahead_fwd_level_t& L) { L.p.hidden = 2000; });
    bad1("mgahead_forward", "momentum=2", hf, hfwd, [](mgahead_fwd_level_t& L) { L.p.momentum = 2.f; });
    bad("mgahead_backward", hb, hbwd); bad_bwd("mgahead_backward", hb, hbwd);
    bad1("mgahead_backward", "gwh NULL", hb, hbwd, [](mgahead_bwd_level_t& L) { L.gwh = nullptr; });
    bad1("mgahead_backward", "eps=0", hb, hbwd, [](mgahead_bwd_level_t& L) { L.p.eps = 0.f; });
    const mgaspade_level_t sp = spade_level(dt, s, 16, 1, 1, true, true, 1, nhwc ? kSpadeNhwc : 0);
    auto sfwd = [](const mgaspade_level_t* L, int n) { return mgaspade_forward(L, n, ST); };
    auto sbwd = [](const mgaspade_level_t* L, int n) { return mgaspade_backward(L, n, ST); };
    bad("mgaspade_forward", sp, sfwd); bad("mgaspade_backward", sp, sbwd); bad_bwd("mgaspade_backward", sp, sbwd);
    for (auto call : {+sfwd, +sbwd}) {
      bad1("mgaspade", "hidden=24", sp, call, [](mgaspade_level_t& L) { L.hidden = 24; });
      bad1("mgaspade", "norm_type=2", sp, call, [](mgaspade_level_t& L) { L.norm_type = 2; });
      bad1("mgaspade", "running_var NULL", sp, call, [](mgaspade_level_t& L) { L.running_var = nullptr; });
      bad1("mgaspade", "wg NULL", sp, call, [](mgaspade_level_t& L) { L.wg = nullptr; });
      bad1("mgaspade", "gwb NULL", sp, call, [](mgaspade_level_t& L) { L.gwb = nullptr; });
      bad1("mgaspade", "y NULL / gy NULL", sp, call, [](mgaspade_level_t& L) { L.y = nullptr; L.gy = nullptr; });
      bad1("mgaspade", "one value per channel", sp, call, [](mgaspade_level_t& L) { L.B = L.H = L.W = 1; });
      bad1("mgaspade", "eps<0", sp, call, [](mgaspade_level_t& L) { L.eps = -1.f; });
    }
  }
  const mgacbam_fwd_level_t cf = cbam_fwd(0, s, 4, 7, true, 0);
  stub_fail_next_launch(); rc("a launch that fails", mgacbam_forward(&cf, 1, ST));
  stub_fail_next_launch(); rc("a plain launch that fails", mgakendall_forward(devf(), 3, devf(), devf(), devf(), ST));
  rc("and the call after it", mgacbam_forward(&cf, 1, ST));
}
static void knob(const char* name, const char* value) {
  printf("knob %s=%s\n", name, value ? value : "(default)");
  if (value) setenv(name, value, 1); else unsetenv(name);
  mgacbam_reload_env();
}
int main(int argc, char** argv) {
  stub_set_occupancy(argc > 1 ? atoi(argv[1]) : 4);
  printf("abi %d occupancy %s\n", mgacbam_abi_version(), argc > 1 ? argv[1] : "4");
  cbam(true); eca(true); head(); spade(); mixed(); loss_side(); invalid();
  const char* knobs[][2] = {{"MGACBAM_BWD_MERGE", "0"}, {"MGACBAM_GATE_NARROW", "1"}, {"MGACBAM_POOL_TX", "32"}, {"MGACBAM_POOL_CPT", "1"},
                            {"MGACBAM_POOL_CPT", "2"}, {"MGACBAM_POOL_CPT", "4"}, {"MGACBAM_CHAN_TX", "16"}, {"MGACBAM_RESIDENT_WGS", "64"},
                            {"MGACBAM_RESIDENT_WGS", "100000"}};
  for (auto& k : knobs) { knob(k[0], k[1]); cbam(false); eca(false); knob(k[0], nullptr); }
  return 0;
}
