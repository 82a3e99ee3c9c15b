// video_dispatch.h - which kernel takes a plan, a frame's plane pointers and a destination, and with which parameters: the gates and
// the parameter builders of the packed path (convert_to_packed of capi_video.cpp), host-only.  The library answers a gate with a launch,
// the emulator (tests/emu/emu_video.cpp) with its lane loops over the same kernel bodies - both call THESE functions, so the CPU tests
// take the device's path by construction.  A gate is the whole condition, plan part and pointer / pitch part together.  What asks the
// device (occupancy, CU count: fused_pick_geometry, col_pick_waves, col_geometry, the strip counts of the bilinear kernels) is not here,
// nor are the on / off knobs: each side reads those from its own source and passes in what a function needs.
#pragma once
#include <cstring>

#include "planner.h"
#include "video_types.h"
#include "video_fast.h"
#include "video_422_fast.h"
#include "video_deep.h"
#include "video_hscale420.h"
#include "video_bilinear_half.h"
#include "video_scale_col.h"
#include "video_swizzle34.h"

namespace gstamd {

inline bool aligned (const void *p, size_t a) { return ((uintptr_t) p & (a - 1)) == 0; }
// every row of an image / plane starts on a multiple of `a` bytes
inline bool rows_aligned (const void *p, int stride, int a) { return aligned (p, (size_t) a) && (stride % a) == 0; }
inline bool plane_aligned (const Planes &pl, int i, int a) { return rows_aligned (pl.p[i], pl.stride[i], a); }

inline bool color_is_none (const ColorParams &c) { return c.matrix.kind == MATRIX_NONE && c.alpha_kind == ALPHA_NONE; }

// chroma rows the vertical upsampler of a 4:2:0 source may touch, relative to the crop: with a source crop it still sees the frame's rows
// above / below the crop (do_unpack_lines :2966)
inline void chroma_row_clamp (const RectPlan &r, int *lo, int *hi)
{
  *lo = -(r.in_y >> 1);
  *hi = ((r.in_maxh + 1) >> 1) - 1 - (r.in_y >> 1);
}

// pack_pos: the plan's own, or the byte order an intermediate image wants
inline FastParams make_fast_params (const VideoPlan &p, bool rgb24 = false, const int *pack_pos = nullptr)
{
  FastParams fp;
  fp.width = p.front.width;
  fp.height = p.front.height;
  fast_params_finish (fp, p.matrix.p, pack_pos ? pack_pos : p.post.pack_pos, p.front.u_plane);
  chroma_row_clamp (p.rect, &fp.crow_lo, &fp.crow_hi);
  if (rgb24)
    fast_params_rgb24 (fp, p.matrix.p, p.fout->pos, p.front.u_plane);
  return fp;
}

// one scaler pass with its tables where the kernels read them (device memory in the library, the plan's vectors in the emulator)
inline ScaleDev make_scale_dev (const ScalePass &sp, const uint32_t *offset, const int16_t *taps, const uint32_t *tapw)
{
  ScaleDev sd;
  sd.kind = sp.kind;
  sd.n_taps = sp.n_taps;
  sd.inc = sp.inc;
  sd.offset = offset;
  sd.taps = taps;
  sd.tapw = tapw;
  sd.nw = sp.nw;
  sd.nw4 = sp.nw4;
  return sd;
}

// ---- unscaled kernels ----

// k_convert_pair / k_convert_strip: dalign 16 for 4-byte pixels, 4 for the 3-byte stores of the rgb24 form
inline bool fast_pair_usable (const VideoPlan &p, const Planes &pl, const uint8_t *dst, int dstride, int dalign = 16)
{
  return p.passes.empty () && p.fast_pair && rows_aligned (dst, dstride, dalign) && plane_aligned (pl, 0, 4) && plane_aligned (pl, 1, 4);
}

inline bool convert420p_usable (const VideoPlan &p, const Planes &pl, const uint8_t *dst, int dstride)
{
  return p.fast_420p && plane_aligned (pl, 0, 8) && aligned (pl.p[1], 4) && aligned (pl.p[2], 4) && (pl.stride[1] % 4) == 0 && pl.stride[1] == pl.stride[2] &&
      rows_aligned (dst, dstride, 16);
}

inline Fast420pParams make_fast420p_params (const VideoPlan &p, const Planes &pl)
{
  Fast420pParams q;
  q.fp = make_fast_params (p);
  q.y = pl.p[0];
  q.u = pl.p[p.front.u_plane];
  q.v = pl.p[p.front.v_plane];
  q.ystride = pl.stride[0];
  q.cstride = pl.stride[1];
  return q;
}

// k_convert422, and its form without a colour stage (k_convert422_ayuv)
inline bool convert422_usable (const VideoPlan &p, bool ayuv, const Planes &pl, const uint8_t *dst, int dstride)
{
  return (ayuv ? p.fast_422_ayuv : p.fast_422) && plane_aligned (pl, 0, 16) && rows_aligned (dst, dstride, 16);
}

inline Fast422Params make_fast422_params (const VideoPlan &p, bool ayuv)
{
  Fast422Params q;
  memset ((void *) &q, 0, sizeof (q));
  if (ayuv) {
    q.fp.width = p.front.width;
    q.fp.height = p.front.height;
  } else
    q.fp = make_fast_params (p);
  q.chroma_h = p.front.chroma_h;
  fast422_selectors (p.front.pos[1], p.front.pos[2], p.front.pos[3], &q);
  return q;
}

// k_swizzle34: a 3- / 4-byte pixel permutation with nothing else in the chain; *sp: the kernel's parameters
inline bool swizzle34_setup (int src_bytes, const int *src_pos, int dst_bytes, const int *dst_pos, const uint8_t *src, int sstride, uint8_t *dst, int dstride,
    int width, Swz34Params *p)
{
  if (!rows_aligned (src, sstride, 4) || !rows_aligned (dst, dstride, 4) || (src_bytes == 4 && dst_bytes == 4))
    return false;
  uint8_t map[4] = {0, 0, 0, 0};
  for (int c = dst_bytes == 4 ? 0 : 1; c < 4; c++)
    map[dst_pos[c]] = c == 0 && src_bytes == 3 ? 0xff : (uint8_t) src_pos[c];
  memset ((void *) p, 0, sizeof (*p));
  if (src_bytes == 3 && dst_bytes == 4)
    swz34_selectors<3, 4> (map, p);
  else if (src_bytes == 4 && dst_bytes == 3)
    swz34_selectors<4, 3> (map, p);
  else
    swz34_selectors<3, 3> (map, p);
  p->src = src, p->sstride = sstride, p->dst = dst, p->dstride = dstride, p->width = width;
  return true;
}

// ... from a 3-byte source into the 4-byte destination of the packed path
inline bool swizzle34_usable (const VideoPlan &p, const ColorParams &color, const Planes &pl, uint8_t *dst, int dstride, Swz34Params *sp)
{
  return p.front.kind == UNPACK_PACKED3 && p.front.hi_depth == 0 && color_is_none (color) &&
      swizzle34_setup (3, p.front.pos, 4, p.post.pack_pos, pl.p[0], pl.stride[0], dst, dstride, p.front.width, sp);
}

// k_swizzle4: 4-byte packed -> 4-byte packed, no matrix, no alpha operation: the copy-shaped permutation kernel
inline bool swizzle4_usable (const FrontParams &f, const Planes &pl, const ColorParams &color, const uint8_t *dst, int dstride)
{
  return f.kind == UNPACK_PACKED4 && f.hi_depth == 0 && color_is_none (color) && rows_aligned (dst, dstride, 16) && plane_aligned (pl, 0, 16);
}

// ---- 10-bit sources ----

// the frames the deep16 rung refuses: 0 none; 1 a three-samples-per-word frame off its 32-bit words; 2 the destination off 4 bytes; 3 a sample
// plane off 2 bytes.  (The byte-stream kinds - NV12_10LE40 & co, UYVP - are read byte by byte: rows of five-byte groups have no alignment.)
inline int deep16_refusal (const VideoPlan &p, const Planes &pl, const uint8_t *dst, int dstride)
{
  const int k = p.front.kind;
  const bool bytes_in = k == UNPACK_SEMI_LE40 || k == UNPACK_P422_UYVP || k == UNPACK_SEMI_LE40_TILED;
  const bool words_in = k == UNPACK_SEMI_LE32 || k == UNPACK_GRAY_LE32;
  if (words_in && (!plane_aligned (pl, 0, 4) || (k == UNPACK_SEMI_LE32 && !plane_aligned (pl, 1, 4))))
    return 1;
  if (!rows_aligned (dst, dstride, 4))
    return 2;
  if (!bytes_in && (!plane_aligned (pl, 0, 2) || !plane_aligned (pl, 1, 2) || (k == UNPACK_PLANAR && !plane_aligned (pl, 2, 2))))
    return 3;
  return 0;
}

// k_front_hscale16: the 16-bit front inside a first, horizontal u16 pass; false: this front has no specialised form (k_front16 + k_scale16)
inline bool front_hscale16_usable (const FrontParams &f, bool fast_on) { return fast_on && deep_front4_variant (f) >= 0; }

// ---- nearest / 2-tap in both directions ----

inline bool scale_small_kind (int k) { return k == SCALE_NEAREST || k == SCALE_2TAP; }
inline bool bilinear_plan (const VideoPlan &p) { return p.passes.size () == 2 && scale_small_kind (p.passes[0].kind) && scale_small_kind (p.passes[1].kind); }

// can the frame's rows go through the vector fetches of the 4:2:0 bilinear kernels?
inline int bil_vec_ok (const BilParams &bp, const Planes &pl)
{
  if (bp.planar)
    /* planar sources only through the straight-line fetch: whole 16-pixel pieces, 8-byte chroma loads */
    return plane_aligned (pl, 0, 16) && plane_aligned (pl, 1, 8) && plane_aligned (pl, 2, 8) && (bp.fp.width % 16) == 0;
  return plane_aligned (pl, 0, 16) && plane_aligned (pl, 1, 16);
}

struct BilKnobs {
  bool on, ayuv_on, table, rows_on, half_on;       // table: the pair table even where it is the closed form
  int tile, rows_tile;                             // outputs per wave of k_bilinear420 / k_bilinear420_rows, < 0: the kernels' own choice
};

// Does the plan take the direct 4:2:0 bilinear kernels (video_bilinear_fast.h / video_bilinear_rows.h / video_bilinear_half.h)?  Fills everything
// of BilParams that does not depend on a particular frame's pointers; voffset / vtaps / vpair: the vertical pass's and the pairing tables as the
// kernels will read them (the checks here read the plan's own copies)
inline bool bilinear420_params (const VideoPlan &p, const BilKnobs &k, const uint32_t *voffset, const int16_t *vtaps, const int *vpair, BilParams *out)
{
  /* no colour stage at all (YUV -> YUV of one colorimetry: the pack image of a planar / semi-planar destination, an AYUV frame): the same kernels
     with the layout that stores A Y U V (GSTAMD_LAYOUT_AYUV) - NV12 4K -> I420 1080p took 65 us through the generic wave-tile scaler */
  const bool ayuv = bilinear420_ayuv_plan (p) && k.ayuv_on;
  if ((p.out_planar && !ayuv) || !bilinear_plan (p))
    return false;
  /* semi-planar / planar 4:2:0 source, horizontal-first 2-tap x 2-tap, fast matrix */
  if (!(p.passes[0].horizontal && p.passes[0].kind == SCALE_2TAP && p.passes[1].kind == SCALE_2TAP && kind_has_planes (p.front.kind) && p.front.w_sub == 1 &&
        p.front.h_sub == 1 && !p.matrix_before_scale && (p.fast_post || ayuv) && p.front.chroma_v2 != 2 && k.on))
    return false;
  const int out_w = p.out_info.width, out_h = p.out_info.height;
  BilParams bp;
  memset (&bp, 0, sizeof (bp));
  bp.tile_w = k.tile >= 0 ? k.tile : bil_pick_tile (out_w, p.passes[0].inc, &bp.ylen);
  if (k.tile >= 0)
    bp.ylen = bil_ylen (out_w, p.passes[0].inc, bp.tile_w);
  if (bp.tile_w <= 0 || bp.ylen <= 0)
    return false;
  bp.fp = make_fast_params (p);
  bp.fp.ayuv = ayuv ? (p.matrix.kind == MATRIX_NONE ? 1 : 2) : 0;
  bp.fp.m8 = p.matrix;
  bp.out_w = out_w;
  bp.out_h = out_h;
  bp.inc = p.passes[0].inc;
  bp.voffset = voffset;
  bp.vtaps = vtaps;
  bp.vpair = p.front.chroma_v2 ? vpair : nullptr;
  bp.planar = p.front.kind == UNPACK_PLANAR;
  bp.u_plane = p.front.u_plane;
  bp.v_plane = p.front.v_plane;
  if (p.front.chroma_v2 && !k.table) {
    /* are the pairs of every source line the kernel will touch the closed form of bil_rows? */
    bool regular = true;
    BilParams probe = bp;
    probe.regular_pairs = 1;
    for (int y = 0; y < out_h && regular; y++)
      for (int l = 0; l < 2 && regular; l++) {
        const int line = (int) p.passes[1].offset[y] + l;
        int ra, rb, role;
        bil_rows (probe, line, &ra, &rb, &role);
        const int e0 = p.vpair[2 * line], ta = vpair_row (e0), trole = vpair_role (e0), tb = p.vpair[2 * line + 1];
        regular = ta == ra && tb == rb && (ra == rb || trole == role);
      }
    bp.regular_pairs = regular ? 1 : 0;
  }
  /* rows per wave of k_bilinear420_rows: every source line pair has to sit in the three-row window of video_bilinear_rows.h */
  if (bp.regular_pairs && (p.front.width % 16) == 0 && k.rows_on) {
    bool fits = true;
    for (int y = 0; y < out_h && fits; y++)
      fits = bilr_window_matches (bp, (int) p.passes[1].offset[y]);
    int rows_ylen = 0;
    bp.rows_tile_w = k.rows_tile >= 0 ? k.rows_tile : bilr_pick_tile (out_w, p.passes[0].inc, &rows_ylen);
    if (k.rows_tile >= 0)
      rows_ylen = bil_ylen (out_w, p.passes[0].inc, bp.rows_tile_w);
    if (fits && bp.rows_tile_w > 0 && rows_ylen > 0)
      bp.rows = -1;           /* as many waves as the device holds at once; a side with a count of its own puts it here */
  }
  bp.half = k.half_on && bilh_plan_ok (bp, p.passes[1].offset.data (), p.passes[1].taps.data ());
  *out = bp;
  return true;
}

// the frame's side of the bilinear rung: 4-byte destination rows; a planar source only where its rows are vectorisable (the kernels have no other
// fetch for three planes) - with this the choice is final, launch_bilinear420 does not refuse
inline bool bilinear420_usable (const BilParams &bp, const Planes &pl, const uint8_t *dst, int dstride)
{
  return rows_aligned (dst, dstride, 4) && (!bp.planar || bil_vec_ok (bp, pl));
}

// the rows kernel takes frames [0, n): every one vectorisable, the destinations 4-byte aligned (bilinear420_usable saw frame 0's pitch)
inline bool bilinear420_rows_usable (const BilParams &bp, int n, const Planes *pl, uint8_t *const *dst)
{
  bool ok = bp.rows != 0 && (bp.fp.width % 16) == 0 && bp.regular_pairs;
  for (int f = 0; f < n && ok; f++)
    ok = bil_vec_ok (bp, pl[f]) && aligned (dst[f], 4);
  return ok;
}

// the exact halving (BilParams::half) on frames [0, n) whose rows are 16-byte aligned.  small_ok: also a single frame of less than 4 M outputs - a
// wave needs a 1024-pixel source column to itself: such a frame is a few hundred waves with long serial walks, and the rows kernel's narrower tiles
// win (4K -> 1080p, one frame: 12.6 us against 15.2; 8K -> 4K: 24.2 against 22.8; in lists this kernel, 14.3 against 18)
inline bool bilinear420_half_usable (const BilParams &bp, int n, const Planes *pl, uint8_t *const *dst, int dstride, bool small_ok)
{
  if (!bp.half || (dstride % 16) != 0)
    return false;
  if (n == 1 && (long) bp.out_w * bp.out_h < 4000000 && !small_ok)
    return false;
  for (int f = 0; f < n; f++) {
    const Planes &q = pl[f];
    if (!plane_aligned (q, 0, 16) || !aligned (dst[f], 16) || q.stride[0] != pl[0].stride[0] || q.stride[1] != pl[0].stride[1] || q.stride[2] != pl[0].stride[2])
      return false;
    if (bp.planar ? (!plane_aligned (q, 1, 8) || !plane_aligned (q, 2, 8)) : !plane_aligned (q, 1, 16))
      return false;
  }
  return true;
}

// k_bilinear4_rows / _up behind a colour stage: enlarging (the matrix runs on the source's pixels, chain_convert ahead of chain_scale) from planes or
// packed 4:2:2 - the source frame goes through the front and the colour stage into an A, c1, c2, c3 image of ITS size, the scaler reads that image
inline bool bilinear4_pre_usable (const VideoPlan &p, const uint8_t *dst, int dstride)
{
  return p.matrix_before_scale && p.front.kind != UNPACK_PACKED4 && p.front.hi_depth == 0 && rows_aligned (dst, dstride, 4);
}

// ... NV12 / NV21: that image is the unscaled conversion into A, R, G, B bytes - the line-pair kernel
inline bool fast_pre_usable (const VideoPlan &p, const Planes &pl) { return p.fast_pre && plane_aligned (pl, 0, 4) && plane_aligned (pl, 1, 4); }

inline FastParams make_fast_pre_params (const VideoPlan &p)
{
  const int ident[4] = {0, 1, 2, 3};
  return make_fast_params (p, false, ident);
}

// ---- N-tap passes ----

// a 4-byte packed source whose unpack is the identity (ARGB, AYUV, and every 4-byte format in plane scaling, where the bytes go through
// raw) with no colour step before the scaler IS an image in the scalers' own layout: the image kernels (wave tiles, k_vscale_pk) take it
// directly instead of the one-lane-per-pixel front kernels
inline bool raw4_source (const VideoPlan &p, const ColorParams &pre, const Planes &pl)
{
  return p.front.kind == UNPACK_PACKED4 && p.front.pos[0] == 0 && p.front.pos[1] == 1 && p.front.pos[2] == 2 && p.front.pos[3] == 3 && color_is_none (pre) &&
      plane_aligned (pl, 0, 4);
}

// the 4:2:0 kernels that filter chroma rows ahead of the blend (k_scale_col, k_scale420_fused, k_hscale420_reg): no colour step ahead of the scaler,
// U and V planes of one pitch
inline bool regular420_frame_ok (const VideoPlan &p, const Planes &pl, const ColorParams &pre)
{
  return color_is_none (pre) && (p.front.kind == UNPACK_SEMI || pl.stride[p.front.u_plane] == pl.stride[p.front.v_plane]);
}

// k_scale_col (video_scale_col.h), the plan's side: both passes N-tap over a regular 4:2:0 source, and a form that holds them
inline bool col_plan_ok (const VideoPlan &p, int opl_pref, bool share, bool regwin, ColTables *t, ColForm *f, int *crow_lo, int *crow_hi)
{
  return col_plan_regular (p, crow_lo, crow_hi) && col_choose (p.passes[0], p.passes[1], p.front.width, p.front.height, opl_pref, share, t, f, regwin);
}

// ... the destination rows: a lane stores its `opl` outputs as one word group
inline bool col_dst_ok (const ColForm &f, const uint8_t *dst, int dstride) { return rows_aligned (dst, dstride, 4 * f.opl); }

// ... ColParams but the launch geometry (rows per wave / workgroup, chunks, tiles, hand-over slots)
inline ColParams make_col_params (const VideoPlan &p, const Planes &pl, int crow_lo, int crow_hi, const int32_t *tiles, const uint32_t *hout, const uint32_t *vrow,
    int dstride)
{
  ColParams q;
  memset ((void *) &q, 0, sizeof (q));
  q.ystride = pl.stride[0];
  q.cstride = p.front.kind == UNPACK_SEMI ? pl.stride[1] : pl.stride[p.front.u_plane];
  q.width = p.front.width;
  q.height = p.front.height;
  q.u_first = p.front.u_plane != 0;
  q.crow_lo = crow_lo;
  q.crow_hi = crow_hi;
  q.tiles = tiles;
  q.hout = hout;
  q.vrow = vrow;
  q.out_w = p.passes[0].out_size;
  q.out_h = p.passes[1].out_size;
  q.dstride = dstride;
  return q;
}

// k_hscale420_reg, the plan's side: first pass horizontal N-tap in byte dot products from a 4:2:0 source whose planner-simulated pair table is the
// closed form of h420r_rows (every line consumed in order).  g0: pass_tile_geom of the first pass
inline bool hscale420_reg_plan_ok (const VideoPlan &p, const TileGeom &g0, int *crow_lo, int *crow_hi)
{
  if (!(p.passes.size () == 2 && p.passes[0].horizontal && p.passes[0].kind == SCALE_NTAP && p.passes[0].dot4_ok && g0.tile16_w > 0 &&
        p.front.chroma_v2 == 1 && kind_has_planes (p.front.kind) && p.front.w_sub == 1 && p.front.h_sub == 1 && !p.matrix_before_scale &&
        (int) p.vpair.size () >= 2 * p.front.height))
    return false;
  chroma_row_clamp (p.rect, crow_lo, crow_hi);
  for (int y = 0; y < p.front.height; y++) {
    int heavy, light;
    h420r_rows (*crow_lo, *crow_hi, y, &heavy, &light);
    const int e0 = p.vpair[2 * y], ta = vpair_row (e0), tb = p.vpair[2 * y + 1];
    const int th = vpair_role (e0) == 0 ? ta : tb, tl = vpair_role (e0) == 0 ? tb : ta;
    if (th != heavy || tl != light)
      return false;
  }
  return true;
}

// ... its parameters, for the two-pass form (dst: the intermediate image) and inside Fused420Params (dst NULL)
inline H420RegParams make_h420_reg_params (const VideoPlan &p, const Planes &pl, int crow_lo, int crow_hi, const ScaleDev &sd0, int tile_w, uint8_t *dst, int dstride)
{
  H420RegParams hp;
  memset (&hp, 0, sizeof (hp));
  hp.y = pl.p[0];
  hp.ystride = pl.stride[0];
  hp.semi = p.front.kind == UNPACK_SEMI;
  hp.u_first = p.front.u_plane != 0;
  hp.c0 = hp.semi ? pl.p[1] : pl.p[p.front.u_plane];
  hp.c1 = hp.semi ? pl.p[1] : pl.p[p.front.v_plane];
  hp.cstride = hp.semi ? pl.stride[1] : pl.stride[p.front.u_plane];
  hp.width = p.front.width;
  hp.height = p.front.height;
  hp.crow_lo = crow_lo;
  hp.crow_hi = crow_hi;
  hp.offset = sd0.offset;
  hp.tapw = sd0.tapw;
  hp.nw4 = sd0.nw4;
  hp.dst = dst;
  hp.dstride = dstride;
  hp.out_w = p.passes[0].out_size;
  hp.tile_w = tile_w;
  return hp;
}

// ... the frame's side, k_scale420_fused's too: 16-pixel pieces of luma, the chroma rows that go with them, 4-byte destination rows, a window of 3 .. 5 words
inline bool hscale420_reg_frame_ok (const H420RegParams &p, int nw, const uint8_t *dst, int dstride)
{
  return (p.width % 16) == 0 && rows_aligned (p.y, p.ystride, 16) && rows_aligned (dst, dstride, 4) && nw >= 3 && nw <= 5 &&
      (p.semi ? rows_aligned (p.c0, p.cstride, 16) : (rows_aligned (p.c0, p.cstride, 8) && aligned (p.c1, 8)));
}

// k_scale420_fused (video_scale420_fused.h), the plan's side: behind hscale420_reg_plan_ok a vertical N-tap second pass whose groups make tables
inline bool fused420_plan_ok (const VideoPlan &p, Fused420Tables *t)
{
  return !p.passes[1].horizontal && p.passes[1].kind == SCALE_NTAP && p.passes[0].nw >= 3 && p.passes[0].nw <= 5 && make_fused420_tables (p.passes[1], p.front.height, t);
}

}  // namespace gstamd
