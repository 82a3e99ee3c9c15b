// tests/emu/emu_audio_many_layouts.cpp - TEST INFRASTRUCTURE: gstamd_audio_converter_samples_many with non-interleaved and wide converters
// in its batched runs on the host the way the device runs it - the walk over the call's streams (aconv_many_run_length of
// audio_convert_plan.h, with the `layouts` flag set), and for every batched run a loop over the grid of each launch through the bodies the
// kernels call: k_aconv_pre_many / _pre_planes_many / _pre_mix_many / k_aconv_wide_mix_many (two phases around its barrier, a host "LDS"
// of the kernel's size), k_aconv_post_many / _post_planes_many, k_aconv_shape_many / _shape_planes_many (64 lanes, lane = stream), with
// the table entries aconv_many_*_entry fill.  Mirrors gstamd_audio_converter_samples_many / aconv_run_many of audio_convert.hip.
// emu_audio_many.cpp stays the twin of the rule without the flag (ordinary converters only); this one's prefix is "emu_aconv_many_layouts_".
//
// The converters are the emulator's existing handles, told apart in kind[] as there: 0 of emu_aconv_planes_new, 1 of emu_aconv_wide_new,
// 3 the latter with a resampler inside.  A stream that is not batched goes through its own emulator's emu_aconv_*_samples.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../gstreamer_amd/csrc/audio_convert_plan.h"
#include "../../gstreamer_amd/csrc/audio_taps.h"

using namespace gstamd;

extern "C" {
void emu_audio_resample (void *h, const void *in, size_t in_frames, void *out, size_t out_frames);
void emu_aconv_planes_samples (void *h, uint8_t *in, size_t in_frames, uint8_t *out, size_t out_frames);
void emu_aconv_wide_samples (void *h, uint8_t *in, size_t in_frames, uint8_t *out, size_t out_frames);
}

// the handle of emu_aconv_planes_new: emu_audio_planes.cpp's definition, repeated token for token (one definition rule) - a change
// there is a change here
struct EmuAConvPlanes {
  AConvPlan plan;
  int in_layout = 0, out_layout = 0, flags = 0;
  GstAmdAudioInfo in, out;
  GstAmdAudioConverterConfig cfg;
  bool resample = false, passthrough = false;
  void *resampler = nullptr;
  AConvDitherState dither = { 0xc2d6038fu, 0u, 0 };
  AConvJump jump;
  std::vector<int32_t> hist = std::vector<int32_t> (8 * GSTAMD_AUDIO_MAX_CHANNELS, 0);
};

namespace {

// the handle of emu_aconv_wide_new.  emu_audio_wide.cpp defines it inside its unnamed namespace, so this is a type of this file's own
// with that one's members in that one's order - a change there is a change here
struct EmuAConvWide {
  AConvWidePlan plan;
  int in_layout = 0, out_layout = 0, flags = 0, in_rate = 0, out_rate = 0;
  GstAmdAudioConverterConfig cfg;
  bool resample = false, passthrough = false;
  void *resampler = nullptr;
  AConvDitherState dither = { 0xc2d6038fu, 0u, 0 };
  AConvJump jump;
  std::vector<int32_t> hist = std::vector<int32_t> (8 * GSTAMD_AUDIO_MAX_CHANNELS_WIDE, 0);
};

thread_local int32_t many_debug[4] = { 0, 0, 0, 0 };

// what gstamd_audio_converter_samples_many reads of a converter, from either handle
struct Conv {
  void *h;
  const AConvPlan *plan;
  const AConvWidePlan *wide_plan;
  bool wide, passthrough;
  int in_layout, out_layout;
  void *resampler;
  AConvDitherState *dither;
  const AConvJump *jump;
  int32_t *hist;
};

Conv conv_of (void *h, int kind)
{
  if (kind & 1) {
    EmuAConvWide *c = (EmuAConvWide *) h;
    return { h, &c->plan.s, &c->plan, true, c->passthrough, c->in_layout, c->out_layout, c->resampler, &c->dither, &c->jump, c->hist.data () };
  }
  EmuAConvPlanes *c = (EmuAConvPlanes *) h;
  return { h, &c->plan, nullptr, false, c->passthrough, c->in_layout, c->out_layout, c->resampler, &c->dither, &c->jump, c->hist.data () };
}

// a stream as aconv_many_run_length sees it
AConvManyItem item_of (const Conv &c, bool has_input, size_t in_frames, size_t out_frames)
{
  return { c.plan, c.h, !c.wide && !c.in_layout && !c.out_layout && !c.passthrough, c.resampler != nullptr, has_input, in_frames, out_frames, true, c.passthrough,
    c.wide, c.in_layout, c.out_layout, c.wide_plan };
}

// aconv_run_many
void many_run (int run, const Conv *cs, const uint8_t *const *in, const size_t *in_frames, uint8_t *const *out, const size_t *out_frames)
{
  const AConvPlan &p = *cs[0].plan;
  const size_t mb = (size_t) amid_bytes (p.mid_in) * (size_t) p.out_ch;
  const bool shape = aconv_plan_shapes (p), resample = cs[0].resampler != nullptr;
  const int out_layout = cs[0].out_layout;
  std::vector<std::vector<uint8_t>> mid_a ((size_t) run), mid_b ((size_t) run);
  std::vector<std::vector<int32_t>> q ((size_t) run);
  for (int k = 0; k < run; k++) {
    mid_a[(size_t) k].assign (in_frames[k] * mb, 0xcd);
    mid_b[(size_t) k].assign ((out_frames[k] ? out_frames[k] : 1) * mb, 0xcd);
    if (shape && out_frames[k])
      q[(size_t) k].assign (out_frames[k] * (size_t) p.out_ch * 2, 0);
  }
  switch (aconv_many_first (p, cs[0].wide, cs[0].in_layout, out_layout)) {
    case ACONV_FIRST_WIDE: {                    /* k_aconv_wide_mix_many: blockIdx.x = tile, blockIdx.y = stream, 256 lanes, a barrier between the phases */
      AConvManyPrePlanesTable t;
      memset ((void *) &t, 0, sizeof (t));
      const int tile = aconv_wide_tile_frames (p.in_ch, p.out_ch);
      std::vector<uint8_t> lds (aconv_wide_lds_bytes (p, tile));
      size_t tiles = 0;
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_wide_entry (in[k], in_frames[k], mid_a[(size_t) k].data (), tile, &t.s[k]);
        tiles = l > tiles ? l : tiles;
      }
      const AConvWidePlan &wp = *cs[0].wide_plan;                               /* the first converter's matrix */
      const AConvWideMatrix w = { wp.m.data (), wp.mi.data (), wp.use.data () };
      for (int y = 0; y < run; y++)
        for (size_t bx = 0; bx < tiles; bx++) {
          const AConvManyPrePlanes &m = t.s[y];
          size_t n0;
          int nf;
          if (!aconv_wide_many_tile (m, bx, tile, &n0, &nf))
            continue;
          std::fill (lds.begin (), lds.end (), (uint8_t) 0xcd);                 /* a workgroup finds LDS as whoever ran before left it */
          uint8_t *x = lds.data (), *mat = lds.data () + aconv_wide_x_bytes (p, tile);
          for (int tid = 0; tid < 256; tid++) {
            if (p.mix)
              aconv_wide_stage_matrix (p, w, mat, tid, 256);
#define PRE(K) aconv_wide_stage_lane<K> (p, aconv_many_side (m.in, akind_bytes (K)), cs[0].in_layout, n0, nf, x, tid, 256)
            GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
          }
          for (int tid = 0; tid < 256; tid++)
            aconv_wide_mix_lane (p, x, mat, w.use, m.mid, n0, nf, tid, 256);
        }
      break;
    }
    case ACONV_FIRST_PLANES: {                  /* k_aconv_pre_planes_many: blockIdx.y = output channel, blockIdx.z = stream */
      AConvManyPrePlanesTable t;
      memset ((void *) &t, 0, sizeof (t));
      size_t lanes = 0;
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_pre_planes_entry (p, in[k], in_frames[k], mid_a[(size_t) k].data (), &t.s[k]);
        lanes = l > lanes ? l : lanes;
      }
      const size_t grid = ((lanes + 255) / 256) * 256;
#define PRE(K) for (int z = 0; z < run; z++) for (int y = 0; y < p.out_ch; y++) for (size_t x = 0; x < grid; x++) aconv_pre_planes_many_lane<K> (p, t.s[z], y, x)
      GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
      break;
    }
    case ACONV_FIRST_MIX: {                     /* k_aconv_pre_mix_many */
      AConvManyPreTable t;
      memset ((void *) &t, 0, sizeof (t));
      size_t lanes = 0;
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_pre_mix_entry (p, in[k], in_frames[k], mid_a[(size_t) k].data (), &t.s[k]);
        lanes = l > lanes ? l : lanes;
      }
      const size_t grid = ((lanes + 255) / 256) * 256;
#define PRE(K) for (int z = 0; z < run; z++) for (int y = 0; y < p.out_ch; y++) for (size_t x = 0; x < grid; x++) aconv_pre_mix_many_lane<K> (p, t.s[z], y, x)
      GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
      break;
    }
    default: {                                  /* k_aconv_pre_many */
      AConvManyPreTable t;
      memset ((void *) &t, 0, sizeof (t));
      size_t lanes = 0;
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_pre_entry (p, in[k], in_frames[k], mid_a[(size_t) k].data (), &t.s[k]);
        lanes = l > lanes ? l : lanes;
      }
      const size_t grid = ((lanes + 255) / 256) * 256;
#define PRE(K) for (int y = 0; y < run; y++) for (size_t x = 0; x < grid; x++) aconv_pre_many_lane<K> (p, t.s[y], x)
      GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
      break;
    }
  }
  many_debug[3]++;
  if (resample)                                 /* gstamd_audio_resampler_resample_many: independent streams, whatever the launch */
    for (int k = 0; k < run; k++)
      emu_audio_resample (cs[k].resampler, mid_a[(size_t) k].data (), in_frames[k], mid_b[(size_t) k].data (), out_frames[k]);
  AConvManyShapeTable sh;
  memset ((void *) &sh, 0, sizeof (sh));
  size_t lanes = 0;
  if (out_layout) {
    AConvManyPostPlanesTable t;
    memset ((void *) &t, 0, sizeof (t));
    for (int k = 0; k < run; k++) {
      int32_t *qk = shape && out_frames[k] ? q[(size_t) k].data () : nullptr;
      const size_t l = aconv_many_post_planes_entry (p, *cs[k].dither, resample ? mid_b[(size_t) k].data () : mid_a[(size_t) k].data (), out[k], out_frames[k], qk, &t.s[k]);
      lanes = l > lanes ? l : lanes;
      sh.s[k] = { qk, cs[k].hist, out[k], out_frames[k] };
    }
    if (lanes) {
      const size_t grid = ((lanes + 255) / 256) * 256;
#define POST(K) for (int z = 0; z < run; z++) for (int y = 0; y < p.out_ch; y++) for (size_t x = 0; x < grid; x++) \
    aconv_post_planes_many_lane<K> (p, *cs[0].jump, t.s[z], y, x)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, POST); /* k_aconv_post_planes_many */
#undef POST
      many_debug[3]++;
      if (shape) {                              /* k_aconv_shape_planes_many: one workgroup, lane = stream */
#define SHAPE(K) for (int lane = 0; lane < 64; lane++) aconv_shape_planes_many_lane<K> (p, sh.s[lane])
        GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
        many_debug[3]++;
      }
    }
  } else {
    AConvManyPostTable t;
    memset ((void *) &t, 0, sizeof (t));
    for (int k = 0; k < run; k++) {
      int32_t *qk = shape && out_frames[k] ? q[(size_t) k].data () : nullptr;
      const size_t l = aconv_many_post_entry (p, *cs[k].dither, resample ? mid_b[(size_t) k].data () : mid_a[(size_t) k].data (), out[k], out_frames[k], qk, &t.s[k]);
      lanes = l > lanes ? l : lanes;
      sh.s[k] = { qk, cs[k].hist, out[k], out_frames[k] };
    }
    if (lanes) {
      const size_t grid = ((lanes + 255) / 256) * 256;
#define POST(K) for (int y = 0; y < run; y++) for (size_t x = 0; x < grid; x++) aconv_post_many_lane<K> (p, *cs[0].jump, t.s[y], x)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, POST); /* k_aconv_post_many */
#undef POST
      many_debug[3]++;
      if (shape) {                              /* k_aconv_shape_many: blockIdx.x = stream, 64 lanes */
#define SHAPE(K) for (int y = 0; y < run; y++) for (int c = 0; c < 64; c++) aconv_shape_many_lane<K> (p, sh.s[y], c)
        GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
        many_debug[3]++;
      }
    }
  }
  for (int k = 0; k < run; k++)
    aconv_dither_advance (p, *cs[k].jump, cs[k].dither, out_frames[k] * (size_t) p.out_ch);
}

}  // namespace

extern "C" {

// gstamd_audio_converter_samples_many over emulator handles; kind[i] as in emu_aconv_many_samples (NULL: all 0).  Returns GSTAMD_OK or
// GSTAMD_ERR_INVALID, as the C ABI does.
int emu_aconv_many_layouts_samples (int n, void *const *handles, const int *kind, uint8_t *const *in, const size_t *in_frames, uint8_t *const *out,
    const size_t *out_frames)
{
  memset (many_debug, 0, sizeof (many_debug));
  if (n < 0 || (n > 0 && (!handles || !in_frames || !out_frames)))
    return GSTAMD_ERR_INVALID;
  std::vector<Conv> convs;
  for (int i = 0; i < n; i++) {
    if (!handles[i] || (out_frames[i] && (!out || !out[i])))
      return GSTAMD_ERR_INVALID;
    convs.push_back (conv_of (handles[i], kind ? kind[i] : 0));
  }
  for (int i = 0; i < n; i++) {
    const Conv &c = convs[(size_t) i];
    if (in_frames[i] == 0)
      continue;
    if (!c.resampler && !(in && in[i]))
      return GSTAMD_ERR_INVALID;
    if (!c.resampler && !c.passthrough && in_frames[i] != out_frames[i])
      return GSTAMD_ERR_INVALID;
  }
  std::vector<AConvManyItem> items;
  std::vector<int> at;
  for (int i = 0; i < n; i++) {
    if (in_frames[i] == 0)
      continue;
    items.push_back (item_of (convs[(size_t) i], in && in[i] != nullptr, in_frames[i], out_frames[i]));
    at.push_back (i);
  }
  const int live = (int) items.size ();
  for (int done = 0; done < live;) {
    const int run = aconv_many_run_length (&items[(size_t) done], live - done);
    if (run < 2) {
      const int i = at[(size_t) done];
      (convs[(size_t) i].wide ? emu_aconv_wide_samples : emu_aconv_planes_samples) (handles[i], in ? in[i] : nullptr, in_frames[i], out ? out[i] : nullptr, out_frames[i]);
      many_debug[2]++;
    } else {
      Conv cs[GSTAMD_ACONV_MANY_MAX];
      const uint8_t *ip[GSTAMD_ACONV_MANY_MAX];
      uint8_t *op[GSTAMD_ACONV_MANY_MAX];
      size_t inf[GSTAMD_ACONV_MANY_MAX], outf[GSTAMD_ACONV_MANY_MAX];
      for (int k = 0; k < run; k++) {
        const int i = at[(size_t) (done + k)];
        cs[k] = convs[(size_t) i];
        ip[k] = in[i];
        op[k] = out ? out[i] : nullptr;
        inf[k] = in_frames[i];
        outf[k] = out_frames[i];
      }
      many_run (run, cs, ip, inf, op, outf);
      many_debug[0]++;
      many_debug[1] += run;
    }
    done += run;
  }
  return GSTAMD_OK;
}

int emu_aconv_many_layouts_debug (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = many_debug[i];
  return 4;
}

// aconv_many_run_length over the same handles, for a test that states the runs: the length of the run that starts at stream 0
int emu_aconv_many_layouts_run_length (int n, void *const *handles, const int *kind, uint8_t *const *in, const size_t *in_frames, const size_t *out_frames)
{
  std::vector<AConvManyItem> items;
  for (int i = 0; i < n; i++)
    items.push_back (item_of (conv_of (handles[i], kind ? kind[i] : 0), in && in[i] != nullptr, in_frames[i], out_frames[i]));
  return aconv_many_run_length (items.data (), n);
}

}  // extern "C"
