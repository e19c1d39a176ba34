// libmgacbam.so, C ABI (include/ext/mgaimage.h): a batch of uint8 images prepared in one launch
#include "host.cuh"
#include "image.cuh"

#include "../../include/ext/mgaimage.h"

static_assert(kImgTilePx == MGAIMG_TILE_PX && kImgTileW == MGAIMG_TILE_W && kImgTileH == MGAIMG_TILE_H && kImgMaxC == MGAIMG_MAX_C,
              "ImgArgs against the ABI");
static_assert(sizeof(mgaimg_desc_t) == 56, "the descriptor's layout (mirrored by _lib.ImageDesc)");

template <typename F>
static auto with_channels(int C, F f) { return with_int<1, 2, 3, 4>(C, f); }

extern "C" int mgaimg_run(const mgaimg_desc_t* D, void* stream) {
  const char* what = "mgaimg_run";
  if (!D) return fail(MGACBAM_E_NULL, "%s: desc is NULL", what);
  if (!D->src || !D->dst) return fail(MGACBAM_E_NULL, "%s: src and dst must not be NULL", what);
  if (D->B < 1 || D->in_h < 1 || D->in_w < 1 || D->out_h < 1 || D->out_w < 1)
    return fail(MGACBAM_E_SHAPE, "%s: B=%d in=%dx%d out=%dx%d (every size at least 1)", what, D->B, D->in_h, D->in_w, D->out_h, D->out_w);
  if (D->C < 1 || D->C > MGAIMG_MAX_C) return fail(MGACBAM_E_SHAPE, "%s: C=%d (1 .. %d)", what, D->C, MGAIMG_MAX_C);
  const long long in_px = static_cast<long long>(D->in_h) * D->in_w, out_px = static_cast<long long>(D->out_h) * D->out_w;
  const long long most = std::max(in_px, out_px), limit = ((1ll << 31) - 1) / (static_cast<long long>(D->B) * D->C);
  if (most > limit)
    return fail(MGACBAM_E_SHAPE, "%s: B=%d C=%d in=%dx%d out=%dx%d: B * C * max(in, out) must stay below 2^31", what, D->B, D->C, D->in_h, D->in_w,
                D->out_h, D->out_w);
  if (int e = check_dtype(what, D->dtype)) return e;
  if (D->flags & ~(MGAIMG_SRC_NHWC | MGAIMG_DST_NHWC | MGAIMG_REVERSE_C)) return fail(MGACBAM_E_ARG, "%s: flags=0x%x has an unknown bit", what, D->flags);
  if (D->reserved != 0) return fail(MGACBAM_E_ARG, "%s: reserved=%d (0)", what, D->reserved);
  if (!aligned_to(D->dst, elem_size(D->dtype)))
    return fail(MGACBAM_E_ALIGN, "%s: dst must be aligned to its element (%zu-byte)", what, elem_size(D->dtype));

  ImgArgs A{};
  A.src = D->src; A.dst = D->dst;
  A.B = D->B; A.in_h = D->in_h; A.in_w = D->in_w; A.out_h = D->out_h; A.out_w = D->out_w;
  A.src_nhwc = (D->flags & MGAIMG_SRC_NHWC) != 0; A.dst_nhwc = (D->flags & MGAIMG_DST_NHWC) != 0; A.reverse = (D->flags & MGAIMG_REVERSE_C) != 0;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int C = D->C;
  if (D->in_h == D->out_h && D->in_w == D->out_w) {
    // the orders agree where a reversal and a change of layout both do nothing: C = 1, or the same layout and no reversal
    A.flat = C == 1 || (A.src_nhwc == A.dst_nhwc && !A.reverse);
    A.tiles = static_cast<int>((in_px + kImgTilePx - 1) / kImgTilePx);
    const long long per = static_cast<long long>(kBlock) * kImgUnroll * kImgVec;
    const long long grid = A.flat ? std::max(1ll, (in_px * D->B * C + per - 1) / per) : static_cast<long long>(D->B) * A.tiles;
    const auto kernel = with_elem(D->dtype, [&](auto t) {
      return with_channels(C, [&](auto c) { return k_img_convert<elem_t<decltype(t)>, decltype(c)::value>; });
    });
    if (int e = launch("k_img_convert", kernel, grid, kBlock, 0, st, A)) return e;
  } else {
    // ~2048 pixels a tile, full rows where they fit: the rows of a full-width tile are one contiguous run
    A.tile_w = std::min(D->out_w, kImgTileW);
    A.tile_h = std::max(1, std::min({D->out_h, kImgTileH, 2048 / A.tile_w}));
    A.tiles_x = (D->out_w + A.tile_w - 1) / A.tile_w;
    A.tiles_y = (D->out_h + A.tile_h - 1) / A.tile_h;
    const long long grid = static_cast<long long>(D->B) * A.tiles_x * A.tiles_y;
    const auto kernel = with_elem(D->dtype, [&](auto t) {
      return with_channels(C, [&](auto c) {
        return with_bool(A.dst_nhwc != 0, [&](auto n) { return k_img_resize<elem_t<decltype(t)>, decltype(c)::value, decltype(n)::value>; });
      });
    });
    if (int e = launch("k_img_resize", kernel, grid, kBlock, 0, st, A)) return e;
  }
  g_err[0] = 0;
  return 0;
}
