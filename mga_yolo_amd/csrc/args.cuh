// Kernel argument blocks (passed by value) and the ctx / scratch layouts shared by host and device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mgacbam {

struct Geo {
  int B, C, H, W, HW;
  int hidden, k;
  int use_sigmoid;
  float thr, eps;
  int proj_h;      // > 0: W1-projection planes of x are saved (forward) / used by k_bwd_apply (backward); = hidden (<= kProjMax in the ctx,
                   // <= kProjWide in the backward's scratch)
};
constexpr int kProjMax = 4;   // MGACBAM_PROJ_MAX_HIDDEN
constexpr int kProjWide = 16; // widest hidden layer the backward makes planes for: the 16 output rows of one v_mfma_f32_16x16x4_f32
constexpr int kGateR = 16;   // channels a thread of the x-resident kernels keeps in registers (x VEC pixels each)
constexpr int kSyncPx = 16;   // a hand-off tile is at least this many pixels: ctx.sync holds ceil(HW/kSyncPx)+1 flags per sample
constexpr int kArriveStride = 64;   // ints between the arrival words of two samples (256 B): returning device-scope adds on ONE line
                                    // serialise at ~90 per us whichever word they hit -- 1,024 of them on one line cost k_pool 7 us

// saved statistics (device pointers into the caller's ctx buffer) -- see mgacbam_ctx_layout_t
struct CtxPtrs {
  float* S; float* use; float* den;
  float* avg; float* mx; float* mavg;
  int* valid; int* amax;
  float* h_avg; float* h_mx; float* ca;
  float* planes; int* cidx; float* sa;
  float* proj;     // (B, hidden, HW) when hidden <= kProjMax (a backward level with wider planes: ScratchPtrs::proj, put here by the host)
  int* sync;       // in-launch hand-off state, all generation counters (zero-filled once by the caller, never reset): [B][nflag] k_gate tile flags,
                   // 4 status words ([0] = time-out), [B] per-sample ca flags, [B][nflag] k_bwd_reduce1 tile flags, [B][nflag] folded conv-tile flags,
                   // ... (host: sync_layout); last, k_pool's arrival words, one per sample, kArriveStride apart (not generation counters: a
                   // launch counts them up and puts them back to 0)
};

struct ParamPtrs { const float* w1; const float* b1; const float* w2; const float* b2; const float* wsa; const float* beta; };

// launch geometry chosen on the host (api.hip: choose_*); TX = lanes along H*W, power of two
struct Tune {
  int pool_tx;     // sweep kernels (k_pool, k_bwd_reduce2, k_eca_*): rows of TX lanes sweep H*W, TY = 256/TX rows x CPT channels
  int pool_cpt;
  int chan_tx;     // tile kernels (k_chan, k_apply, k_bwd_reduce1, k_bwd_apply, k_eca_bwd): one H*W vector per lane, TY = 256/TX channel slices
  int conv_twq;    // backward conv tiles: TWQ quads (4 px) wide, TH rows
  int conv_th;
  int wsa_th;      // k_bwd_wsa tiles: fewer rows so 4 staged planes stay under ~16 KB of LDS (role workgroups)
  int apply_rows;  // k_apply: upper bound of the plane rows (tile rows + halo) staged per workgroup
  int gate_rows;   // k_gate: upper bound of the plane rows (tile rows + halo) staged per workgroup
  int gate_tx;     // k_gate (x-resident chan+apply): TX lanes along H*W, TY = 256/TX slices of kGateR channels each; 0 = not eligible
  int gate_span;   // k_gate: tiles a k x k window reaches on either side (a tile waits for workgroups up to 8*span ids away)
};

// channels-last levels (nhwc.cuh): chunk geometry, a function of the level alone (host: nhwc_geo)
struct NhwcGeo {
  int cs, lcs;     // lanes per pixel (power of two <= 64) and its log2
  int ng;          // channel groups of VEC channels: ceil(C / VEC)
  int ch;          // pixels per TILE = (256 / cs) * pixels per thread (8; 4 with 8-element lanes)
  int ntile;       // tiles per sample: the per-pixel kernels (k_chan_nhwc, k_apply_nhwc, k_bwd_apply_nhwc) take one tile per workgroup
  int rp;          // tiles per CHUNK: the per-channel kernels (k_pool_nhwc, k_bwd_reduce1_nhwc, k_bwd_reduce2_nhwc) sweep rp tiles per
                   // workgroup and write one partial per chunk, so a sample has at most kNhwcMaxChunks partials to fold
  int nchunk;      // chunks per sample = ceil(ntile / rp)
};
constexpr int kNhwcMaxChunks = 64;
constexpr int kNhwcFoldC = 64;   // channels per workgroup of the NHWC fold kernels (x 4 chunk groups = 256 threads)

struct FwdArgs {
  const void* x; const float* mask; void* y;
  CtxPtrs c; ParamPtrs p; Geo g; Tune t;
  int nflag;       // flags per sample in c.sync (host: sync_layout)
  int fused;       // MGACBAM_FWD_FUSE path selected for this level's group
  unsigned spin_limit;   // bound of every hand-off spin (knob MGACBAM_SPIN_LIMIT, default 2^20 ~ 1 s)
  int fault;       // fault injection for tests (knob MGACBAM_FAULT=1): sample 0's role workgroup never publishes ca
  long long* trace;   // MGACBAM_TRACE builds only: per-workgroup phase timestamps (tools/trace_gate.py), else nullptr
  int pool_mlp;    // ca, h_avg, h_mx of this level are formed by k_pool's last arriver of each sample (host: pool_forms_ca, a rule of the
                   // level alone): k_gate gives it no role workgroups and its tiles do not wait for ca
  int arrive0;     // the level's arrival words of k_pool in c.sync (ints), sample b's at arrive0 + b * kArriveStride: 0 between launches
  // channels-last levels (MGACBAM_LAYOUT_NHWC: the kernels of nhwc_fwd.cuh) only
  NhwcGeo n;
  float* ws;       // (B, nchunk, 4*C + 4) pool partials: [sum x*s][sum x][max][arg-max pixel (int)][sum s, 3 pad]
};

// transient backward buffers (device pointers into the caller's scratch buffer)
struct ScratchPtrs {
  float* A_part;    // (B,nt,2,C) per hw-tile partials: [0] A = sum gy*x*sa, [1] D = sum gy*(v-x) (k_bwd_reduce1 -> k_bwd_reduce2)
  float* gpre;      // (B,HW)    dL/d(conv output)
  float* gplanes;   // (B,3,HW)  dL/d(planes)
  float* gwsa_part; // (nconv, 3*k*k)
  float* gz;        // (B,C)     dL/dz
  float* gbq;       // (B,C)     D = sum_hw gy*(v - x)  (for dL/dbeta)
  float* gh_avg;    // (B,hidden)
  float* gh_mx;     // (B,hidden)
  float* pgh;       // (B,ncg,hidden) per-channel-group partials of W2^T g_z (k_bwd_reduce2 -> k_bwd_apply prologue)
  float* proj;      // (B,hidden,HW) W1-projection planes of a level with kProjMax < hidden <= kProjWide (k_bwd_reduce1 tiles -> k_bwd_apply)
};

struct BwdArgs {
  const void* x; const float* mask; const void* gy; void* gx; float* gmask;
  float* gw1; float* gb1; float* gw2; float* gb2; float* gwsa; float* gbeta;
  CtxPtrs c; ParamPtrs p; ScratchPtrs s; Geo g; Tune t;
  int nt;       // hw tiles of k_bwd_reduce1
  int nconv;    // k_bwd_convT tiles of this level (B * tiles_y * tiles_x)
  int nwsa;     // k_bwd_wsa tiles of this level: one dWsa partial each
  int npg;      // parameter-gradient workgroups of this level (k_bwd_params roles)
  int ncg;      // channel groups per sample of k_bwd_reduce2
  int nflag;    // flags per sample in c.sync
  int bflag0;   // first backward hand-off flag in c.sync (ints): [B][nflag], one per k_bwd_reduce1 tile
  int cflag0;   // first flag of the folded transposed-conv tiles in c.sync: [nconv], generation counters like the tile flags
  int wflag0;   // ... of the dWsa tile roles when they ride in the merged launch: [nwsa]
  int sflag0;   // ... of k_bwd_reduce2's sweep workgroups in the merged launch: [B][C], one counter per CHANNEL (a sweep reads its first
                // channel's, bumps all of its own): the channel grouping depends on the call's other levels, the counts do not
  int mbflag0, mcflag0;   // the merged launch's own tile / conv-tile flags (the host puts them into bflag0 / cflag0 for that launch)
  int make_proj;   // > 0: g.proj_h > 0 and the k_bwd_reduce1 tiles write the level's W1-projection planes (0 with MGACBAM_BWD_HAVE_PROJ: the
                   // forward did) -- 1: proj_h <= kProjMax, VALU form; 2: proj_h <= kProjWide, MFMA form (bwd.cuh)
  int merged;   // 1: k_bwd_reduce1 tiles, transposed-conv tiles, dWsa tiles and k_bwd_reduce2 sweeps are ONE launch (k_bwd_r12)
  unsigned spin_limit;
  int vec;      // elements per lane of the tile kernels (TP = chan_tx * vec pixels per tile)
  long long* trace;   // MGACBAM_TRACE builds only (tools/trace_gate.py), else nullptr
  // channels-last levels (MGACBAM_LAYOUT_NHWC: the kernels of nhwc_bwd.cuh) only; their A_part is (B, nchunk, 3, C) = [A][D][sum x*wgt]
  NhwcGeo n;
  int ncb;         // channel blocks of kNhwcFoldC (k_bwd_fold_nhwc): s.pgh is (B, ncb, hidden)
};

static inline size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

// One launch covers up to kGroupMax pyramid levels: workgroup ids [start[l], start[l+1]) belong to level l.
// P3+P4+P5 of YOLOv8n are 52+26+13 MB -- alone, P5 cannot fill 256 CUs and every extra launch costs ~2.5 us of
// dependent-kernel boundary, so each stage is ONE launch whose grid is the concatenation of the levels' grids, the level
// whose workgroups run longest FIRST (api: for_each_group).  Interleaving the levels round-robin instead was measured and
// is worse (k_bwd_reduce1 30 -> 43 us): the long, latency-bound P5 workgroups then also sit in the last round = the tail.
constexpr int kGroupMax = 4;
template <typename Args>
struct Group {
  int n;
  int start[kGroupMax + 1];
  Args lv[kGroupMax];
};
// a launch's arguments may take this many bytes; every group, and every struct that holds one, is checked where it is defined
constexpr size_t kKernargMax = 4096;
static_assert(sizeof(Group<FwdArgs>) <= kKernargMax && sizeof(Group<BwdArgs>) <= kKernargMax, "a group is one launch's arguments");

}  // namespace mgacbam
