// A batch of uint8 images prepared in one launch (include/ext/mgaimage.h states the rule): /255, element type, layout, channel order, and
// the bilinear resize of multi-scale training.
//   k_img_convert: no resize.  A streaming kernel bound by bytes; what matters is the shape of its accesses: every load and store
//                  instruction of a wave covers ONE contiguous range, 4 bytes a lane in, 4 elements (16 / 8 bytes) a lane out.  The flat form
//                  streams the whole batch; the tile form turns the order round through LDS.
//   k_img_resize:  one destination tile per workgroup; the rows' and columns' taps and weights and the 256 quotients v / 255 sit in LDS; the
//                  source bytes are gathered through the cache (the source is a quarter of the fp32 image and a tile's bytes are
//                  read one to four times each, by neighbouring lanes); the stores are those of k_img_convert.
// The source has no alignment: a 4-byte load of it is spelled as a memcpy, which the compiler emits as one global_load_dword (the target
// allows unaligned global accesses); the destination's vectors start where IT is aligned to them.
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr int kImgVec = 4;            // elements a lane stores at once = source bytes a lane loads at once
constexpr int kImgUnroll = 4;         // independent vectors of a lane in the flat form: 4096 elements a workgroup
constexpr int kImgTilePx = 1024;      // = MGAIMG_TILE_PX
constexpr int kImgTileW = 1024;       // = MGAIMG_TILE_W
constexpr int kImgTileH = 64;         // = MGAIMG_TILE_H
constexpr int kImgMaxC = 4;           // = MGAIMG_MAX_C

struct ImgArgs {
  const uint8_t* src;
  void* dst;
  int B, in_h, in_w, out_h, out_w;
  int src_nhwc, dst_nhwc, reverse;
  int flat;                           // k_img_convert: source and destination order agree
  int tiles;                          // k_img_convert, tile form: tiles of kImgTilePx pixels a sample
  int tile_h, tile_w, tiles_y, tiles_x;   // k_img_resize
};

__device__ __forceinline__ unsigned img_ld4(const uint8_t* p) {
  unsigned v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
// the fp32 quotient v / 255, correctly rounded: the taps of the resize, as the rule and its oracle state them
__device__ __forceinline__ float img_unit(unsigned byte) { return static_cast<float>(byte) / 255.0f; }
// what torch's `x / 255` is ON THE DEVICE: a tensor divided by a host scalar is multiplied by the scalar's fp32 reciprocal there (on the host
// it is the quotient).  In fp32 the product differs from the quotient by one ulp for 126 of the 256 bytes; rounded to fp16 or bf16 the two
// agree for all 256.  The no-resize kernel stands in for that composition bit for bit, so it forms the product.
__device__ __forceinline__ float img_unit_device(unsigned byte) { return static_cast<float>(byte) * (1.0f / 255.0f); }

// elements in front of p's first aligned vector (p is aligned to its element: checked on the host)
template <typename T>
__device__ __forceinline__ int img_head(const T* p, long long len) {
  constexpr unsigned vb = sizeof(T) * kImgVec;
  const unsigned mis = static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) % vb);
  const long long h = ((vb - mis) % vb) / sizeof(T);
  return static_cast<int>(h < len ? h : len);
}

// The workgroup writes the contiguous run d[0 .. len): aligned vectors of kImgVec elements, lane after lane, and the elements before the
// first and behind the last of them one by one.  make(e) positions a cursor at element e; cur.get() is its value, cur.next() moves on by one.
template <typename T, typename Make>
__device__ __forceinline__ void img_emit(T* d, int len, int tid, Make make) {
  const int head = img_head(d, len);
  const int nvec = (len - head) / kImgVec;
  for (int k = tid; k < nvec; k += kBlock) {
    const int e = head + k * kImgVec;
    auto cur = make(e);
    float v[kImgVec];
#pragma unroll
    for (int i = 0; i < kImgVec; ++i) { v[i] = cur.get(); cur.next(); }
    store_vec<T, kImgVec>(d + e, v);
  }
  const int rest = len - nvec * kImgVec;                       // head + tail: at most 2 * (kImgVec - 1)
  if (tid < rest) {
    const int e = tid < head ? tid : nvec * kImgVec + tid;
    auto cur = make(e);
    d[e] = from_f32<T>(cur.get());
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// no resize
// ------------------------------------------------------------------------------------------------------------------------------------
template <int C>
struct ImgTileCursor {             // the tile form's destination order over the bytes in LDS
  const uint8_t* lds;
  int p, c;                        // pixel of the tile, DESTINATION channel
  bool src_nhwc, dst_nhwc, reverse;
  __device__ __forceinline__ float get() const {
    const int cs = reverse ? C - 1 - c : c;
    return img_unit_device(lds[src_nhwc ? p * C + cs : cs * kImgTilePx + p]);
  }
  __device__ __forceinline__ void next() {
    if (!dst_nhwc) { ++p; return; }
    if (++c == C) { c = 0; ++p; }
  }
};

template <typename T, int C>
__global__ __launch_bounds__(kBlock) void k_img_convert(const ImgArgs A) {
  const int tid = static_cast<int>(threadIdx.x);
  T* dst = static_cast<T*>(A.dst);
  const long long n = static_cast<long long>(A.in_h) * A.in_w;
  if (A.flat) {
    const long long N = static_cast<long long>(A.B) * C * n;
    const int head = img_head(dst, N);
    const long long nvec = (N - head) / kImgVec;
    const long long k0 = static_cast<long long>(blockIdx.x) * (kBlock * kImgUnroll) + tid;
    unsigned w[kImgUnroll];
#pragma unroll
    for (int u = 0; u < kImgUnroll; ++u) {
      const long long k = k0 + u * kBlock;
      w[u] = k < nvec ? img_ld4(A.src + head + k * kImgVec) : 0u;
    }
#pragma unroll
    for (int u = 0; u < kImgUnroll; ++u) {
      const long long k = k0 + u * kBlock;
      if (k >= nvec) continue;
      float v[kImgVec];
#pragma unroll
      for (int i = 0; i < kImgVec; ++i) v[i] = img_unit_device((w[u] >> (8 * i)) & 0xFFu);
      store_vec<T, kImgVec>(dst + head + k * kImgVec, v);
    }
    if (blockIdx.x == 0) {
      const int rest = static_cast<int>(N - nvec * kImgVec);
      if (tid < rest) {
        const long long e = tid < head ? tid : nvec * kImgVec + tid;
        dst[e] = from_f32<T>(img_unit_device(A.src[e]));
      }
    }
    return;
  }
  // tile form: kImgTilePx pixels of one sample through LDS, in SOURCE order there
  __shared__ __attribute__((aligned(16))) uint8_t lds[C * kImgTilePx];
  const int b = static_cast<int>(blockIdx.x) / A.tiles, t = static_cast<int>(blockIdx.x) - b * A.tiles;
  const long long p0 = static_cast<long long>(t) * kImgTilePx;
  const int np = static_cast<int>(n - p0 < kImgTilePx ? n - p0 : kImgTilePx);
  const uint8_t* sb = A.src + static_cast<long long>(b) * C * n;
  const int runs = A.src_nhwc ? 1 : C, run_len = A.src_nhwc ? np * C : np;
  for (int r = 0; r < runs; ++r) {
    const uint8_t* g = A.src_nhwc ? sb + p0 * C : sb + r * n + p0;
    uint8_t* l = lds + r * kImgTilePx;
    const int nw = run_len / 4;
    for (int k = tid; k < nw; k += kBlock) reinterpret_cast<unsigned*>(l)[k] = img_ld4(g + 4 * k);
    const int e = nw * 4 + tid;
    if (e < run_len) l[e] = g[e];
  }
  __syncthreads();
  const bool sn = A.src_nhwc != 0, dn = A.dst_nhwc != 0, rev = A.reverse != 0;
  if (dn) {
    img_emit(dst + (static_cast<long long>(b) * n + p0) * C, np * C, tid,
             [&](int e) { return ImgTileCursor<C>{lds, e / C, e % C, sn, true, rev}; });
  } else {
    for (int c = 0; c < C; ++c)
      img_emit(dst + (static_cast<long long>(b) * C + c) * n + p0, np, tid, [&](int e) { return ImgTileCursor<C>{lds, e, c, sn, false, rev}; });
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// bilinear resize
// ------------------------------------------------------------------------------------------------------------------------------------
struct ImgTap { int o0, o1; float lam; };     // byte offsets of the two taps along one axis (inside a sample's channel) and the weight

template <int C, bool DST_NHWC>
struct ImgResizeCursor {
  const uint8_t* sb;               // the sample's source bytes
  const float* lut;
  const ImgTap* ytab;
  const ImgTap* xtab;
  int cstride;                     // source bytes between two channels
  int tw;                          // columns of the tile
  int yl, xl, c;                   // row and column of the tile, DESTINATION channel
  bool reverse;
  __device__ __forceinline__ float get() const {
    const uint8_t* s = sb + (reverse ? C - 1 - c : c) * cstride;
    const ImgTap ty = ytab[yl], tx = xtab[xl];
    const float t00 = lut[s[ty.o0 + tx.o0]], t01 = lut[s[ty.o0 + tx.o1]];
    const float t10 = lut[s[ty.o1 + tx.o0]], t11 = lut[s[ty.o1 + tx.o1]];
    const float top = fmaf(tx.lam, t01, (1.f - tx.lam) * t00);
    const float bot = fmaf(tx.lam, t11, (1.f - tx.lam) * t10);
    return fmaf(1.f - ty.lam, top, ty.lam * bot);
  }
  __device__ __forceinline__ void next() {
    if (DST_NHWC && ++c < C) return;
    if (DST_NHWC) c = 0;
    if (++xl == tw) { xl = 0; ++yl; }
  }
};

template <typename T, int C, bool DST_NHWC>
__global__ __launch_bounds__(kBlock) void k_img_resize(const ImgArgs A) {
  __shared__ float lut[256];
  __shared__ ImgTap ytab[kImgTileH];
  __shared__ ImgTap xtab[kImgTileW];
  const int tid = static_cast<int>(threadIdx.x);
  const int per = A.tiles_y * A.tiles_x;
  const int b = static_cast<int>(blockIdx.x) / per, q = static_cast<int>(blockIdx.x) - b * per;
  const int y0 = (q / A.tiles_x) * A.tile_h, x0 = (q % A.tiles_x) * A.tile_w;
  const int th = min(A.tile_h, A.out_h - y0), tw = min(A.tile_w, A.out_w - x0);
  const int pstride = A.src_nhwc ? C : 1;                        // source bytes between two pixels of a row
  const int cstride = A.src_nhwc ? 1 : A.in_h * A.in_w;
  const float sh = static_cast<float>(A.in_h) / static_cast<float>(A.out_h), sw = static_cast<float>(A.in_w) / static_cast<float>(A.out_w);
  lut[tid] = img_unit(static_cast<unsigned>(tid));
  for (int j = tid; j < th + tw; j += kBlock) {
    int i0, i1;
    float lam;
    if (j < th) {
      bilinear_tap(sh, y0 + j, A.in_h, i0, i1, lam);
      ytab[j] = ImgTap{i0 * A.in_w * pstride, i1 * A.in_w * pstride, lam};
    } else {
      bilinear_tap(sw, x0 + j - th, A.in_w, i0, i1, lam);
      xtab[j - th] = ImgTap{i0 * pstride, i1 * pstride, lam};
    }
  }
  __syncthreads();
  const uint8_t* sb = A.src + static_cast<long long>(b) * C * A.in_h * A.in_w;
  T* dst = static_cast<T*>(A.dst);
  const bool rev = A.reverse != 0;
  const long long on = static_cast<long long>(A.out_h) * A.out_w;
  // a full-width tile is one contiguous run per channel (NCHW) or altogether (channels-last); a column strip is one run per row
  const bool full = tw == A.out_w;
  const int rows = full ? 1 : th, run_px = full ? th * tw : tw;
  for (int r = 0; r < rows; ++r) {
    const long long px = static_cast<long long>(y0 + r) * A.out_w + x0;       // first destination pixel of the run
    if constexpr (DST_NHWC) {
      img_emit(dst + (static_cast<long long>(b) * on + px) * C, run_px * C, tid, [&](int e) {
        const int p = e / C;
        return ImgResizeCursor<C, true>{sb, lut, ytab, xtab, cstride, tw, r + p / tw, p % tw, e - p * C, rev};
      });
    } else {
      for (int c = 0; c < C; ++c)
        img_emit(dst + (static_cast<long long>(b) * C + c) * on + px, run_px, tid,
                 [&](int e) { return ImgResizeCursor<C, false>{sb, lut, ytab, xtab, cstride, tw, r + e / tw, e % tw, c, rev}; });
    }
  }
}

}  // namespace mgacbam
