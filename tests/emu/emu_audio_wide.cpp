// tests/emu/emu_audio_wide.cpp - TEST INFRASTRUCTURE: the wide audio converter (gstamd_audio_converter_new_wide, 1 .. 64 channels, DESIGN
// 3.8.3) on the host the way the device runs it - the plan of aconv_make_plan_wide, and a loop over the tiles and lanes of each launch:
// k_aconv_wide_mix as its two phases around the barrier (aconv_wide_stage_matrix + aconv_wide_stage_lane into a host "LDS" of the kernel's
// size, then aconv_wide_mix_lane), k_aconv_pre / k_aconv_post / k_aconv_shape for the unmixed interleaved sides, k_aconv_wide_post_planes
// / _shape_planes for a non-interleaved output.  Mirrors aconv_run of audio_convert.hip for a wide converter.  Prefix "emu_aconv_wide_".
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../gstreamer_amd/csrc/audio_convert_plan.h"
#include "../../gstreamer_amd/csrc/audio_taps.h"
#include "emu_audio_handles.h"

using namespace gstamd;

extern "C" {
void *emu_audio_new (int method, int flags, int format, int channels, int in_rate, int out_rate, const GstAmdAudioResamplerOptions *options, int *status, char *err,
    int err_len);
void emu_audio_free (void *h);
size_t emu_audio_get_out_frames (void *h, size_t in_frames);
void emu_audio_resample (void *h, const void *in, size_t in_frames, void *out, size_t out_frames);
}

namespace {

void *wide_new_resampler (EmuAConvWide *c, char *err, int err_len)
{
  GstAmdAudioResamplerOptions ro;
  if (c->cfg.has_resampler_options)
    ro = c->cfg.resampler_options;
  else
    audio_options_init (&ro);
  int st = 0;
  return emu_audio_new (c->cfg.resampler_method, (c->flags & 2) ? 4 : 0, c->plan.s.mid_in, c->plan.s.out_ch, c->in_rate, c->out_rate, &ro, &st, err, err_len);
}

bool wide_contiguous (uint8_t *const *pl, int n, size_t plane_bytes)
{
  for (int c = 1; c < n; c++)
    if (pl[c] != pl[c - 1] + plane_bytes)
      return false;
  return true;
}

void wide_run (EmuAConvWide *c, uint8_t *const *in, size_t in_frames, uint8_t *const *out, size_t out_frames)
{
  const AConvPlan &p = c->plan.s;
  const size_t in_b = (size_t) afmt_bytes (p.in_fmt), out_b = (size_t) afmt_bytes (p.out_fmt);
  if (in_frames == 0)
    return;
  if (c->passthrough || p.endian_swap) {
    int blocks = c->out_layout ? p.out_ch : 1;
    size_t n = out_frames * (size_t) (c->out_layout ? 1 : p.out_ch);
    if (blocks > 1 && wide_contiguous (in, blocks, n * in_b) && wide_contiguous (out, blocks, n * out_b)) {
      n *= (size_t) blocks;
      blocks = 1;
    }
    for (int b = 0; b < blocks; b++) {
      if (c->passthrough) {
        memmove (out[b], in[b], n * out_b);
        continue;
      }
      const AConvSplit s = aconv_swap_split (in[b], out[b], p.endian_swap, n);           /* k_aconv_swap */
      for (size_t t = 0; t < aconv_split_lanes (s); t++)
        switch (p.endian_swap) {
          case 2: aconv_swap_lane<AK_2LE> (in[b], out[b], s, t); break;
          case 3: aconv_swap_lane<AK_3LE> (in[b], out[b], s, t); break;
          case 4: aconv_swap_lane<AK_4LE> (in[b], out[b], s, t); break;
          default: aconv_swap_lane<AK_8LE> (in[b], out[b], s, t); break;
        }
    }
    return;
  }
  const size_t mb = (size_t) amid_bytes (p.mid_in) * (size_t) p.out_ch;
  std::vector<uint8_t> a ((in_frames ? in_frames : 1) * mb), b ((out_frames ? out_frames : 1) * mb);
  uint8_t *ma = a.data (), *mbuf = b.data ();
  if (in && (c->in_layout || p.mix)) {          /* k_aconv_wide_mix: blockIdx.x = tile, 256 lanes, a barrier between the two phases */
    AConvPlanesWide src;
    memset (&src, 0, sizeof (src));
    for (int ci = 0; ci < (c->in_layout ? p.in_ch : 1); ci++)
      src.p[ci] = in[ci];
    src.frames = in_frames;
    const AConvWideMatrix w = { c->plan.m.data (), c->plan.mi.data (), c->plan.use.data () };
    const int tile = aconv_wide_tile_frames (p.in_ch, p.out_ch);
    std::vector<uint8_t> lds (aconv_wide_lds_bytes (p, tile));
    for (size_t n0 = 0; n0 < in_frames; n0 += (size_t) tile) {
      const int nf = in_frames - n0 < (size_t) tile ? (int) (in_frames - n0) : tile;
      std::fill (lds.begin (), lds.end (), (uint8_t) 0xcd);                     /* a workgroup finds LDS as whoever ran before left it */
      uint8_t *x = lds.data (), *mat = lds.data () + aconv_wide_x_bytes (p, tile);
      for (int tid = 0; tid < 256; tid++) {
        if (p.mix)
          aconv_wide_stage_matrix (p, w, mat, tid, 256);
#define PRE(K) aconv_wide_stage_lane<K> (p, src, c->in_layout, n0, nf, x, tid, 256)
        GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
      }
      for (int tid = 0; tid < 256; tid++)
        aconv_wide_mix_lane (p, x, mat, w.use, ma, n0, nf, tid, 256);
    }
  } else if (in) {                              /* k_aconv_pre */
    const AConvSplit s = aconv_split (in[0], (int) in_b, in_frames * (size_t) p.out_ch, aconv_pre_grouped (p));
#define PRE(K) for (size_t t = 0; t < aconv_split_lanes (s); t++) aconv_pre_lane<K> (p, in[0], ma, s, t)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }
  const uint8_t *after = ma;
  if (c->resampler) {
    emu_audio_resample (c->resampler, in ? ma : nullptr, in_frames, mbuf, out_frames);
    after = mbuf;
  }
  const size_t samples = out_frames * (size_t) p.out_ch;
  if (samples == 0)
    return;
  std::vector<int32_t> qv (samples + 1), qd (samples + 1);
  const bool shape = p.ns && p.quant_shift > 0;
  if (c->out_layout) {                          /* k_aconv_wide_post_planes, k_aconv_wide_shape_planes */
    AConvPlanesWide dst;
    memset (&dst, 0, sizeof (dst));
    for (int co = 0; co < p.out_ch; co++)
      dst.p[co] = out[co];
    dst.frames = out_frames;
    aconv_planes_heads_wide (&dst, p.out_ch, (int) out_b, aconv_post_grouped (p));
    const size_t lanes = aconv_planes_lanes_wide (dst, p.out_ch);
#define POST(K) for (int co = 0; co < p.out_ch; co++) for (size_t t = 0; t < ((lanes + 255) / 256) * 256; t++) \
    aconv_post_lane_planes_of<K> (p, c->jump, c->dither, after, dst, qv.data (), qd.data (), co, t)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
    if (shape) {
#define SHAPE(K) aconv_shape_planes_of<K> (p, qv.data (), qd.data (), c->hist.data (), dst)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
    }
  } else {                                      /* k_aconv_post, k_aconv_shape (64 lanes: one per channel) */
    const AConvSplit s = aconv_split (out[0], (int) out_b, samples, aconv_post_grouped (p));
#define POST(K) for (size_t t = 0; t < aconv_split_lanes (s); t++) aconv_post_lane<K> (p, c->jump, c->dither, after, out[0], qv.data (), qd.data (), s, t)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
    if (shape) {
#define SHAPE(K) for (int ch = 0; ch < 64; ch++) if (ch < p.out_ch) aconv_shape_channel<K> (p, qv.data (), qd.data (), c->hist.data (), out[0], out_frames, ch)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
    }
  }
  aconv_dither_advance (p, c->jump, &c->dither, samples);
}

}  // namespace

extern "C" {

// mix_matrix: NULL, or [out][in]
void *emu_aconv_wide_new (int flags, const GstAmdAudioInfoWide *in, int in_layout, const GstAmdAudioInfoWide *out, int out_layout, const GstAmdAudioConverterConfig *cfg,
    const float *mix_matrix, char *err, int err_len)
{
  auto refuse = [&](const std::string &e) -> void * {
    if (err)
      strncpy (err, e.c_str (), err_len - 1);
    return nullptr;
  };
  if (!in || !out)
    return refuse ("NULL info");
  EmuAConvWide *c = new EmuAConvWide ();
  std::string e;
  c->flags = flags;
  c->in_layout = in_layout;
  c->out_layout = out_layout;
  c->in_rate = in->rate;
  c->out_rate = out->rate;
  c->cfg = *cfg;
  if (aconv_make_plan_wide (flags, in, in_layout, out, out_layout, *cfg, mix_matrix, &c->plan, &c->resample, &c->passthrough, &e) != GSTAMD_OK) {
    delete c;
    return refuse (e);
  }
  if (c->resample && !(c->resampler = wide_new_resampler (c, err, err_len))) {
    delete c;
    return nullptr;
  }
  aconv_make_jump (&c->jump);
  return c;
}

void emu_aconv_wide_free (void *h)
{
  EmuAConvWide *c = (EmuAConvWide *) h;
  if (c && c->resampler)
    emu_audio_free (c->resampler);
  delete c;
}

size_t emu_aconv_wide_get_out_frames (void *h, size_t in_frames)
{
  EmuAConvWide *c = (EmuAConvWide *) h;
  return c->resampler ? emu_audio_get_out_frames (c->resampler, in_frames) : in_frames;
}

int emu_aconv_wide_is_passthrough (void *h) { return ((EmuAConvWide *) h)->passthrough ? 1 : 0; }

int emu_aconv_wide_get_mix_matrix (void *h, float *matrix, int max)
{
  EmuAConvWide *c = (EmuAConvWide *) h;
  const int n = c->plan.s.in_ch * c->plan.s.out_ch;
  for (int i = 0; i < n && i < max; i++)
    matrix[i] = c->plan.m[(size_t) i];
  return n;
}

// frames of a tile of the mixing kernel (the tests put a tile edge inside a run)
int emu_aconv_wide_tile_frames (int in_ch, int out_ch) { return aconv_wide_tile_frames (in_ch, out_ch); }

// the plan's sparse decision and use[] masks (what the tests of the half-full matrix row look at)
int emu_aconv_wide_sparse (void *h, uint64_t *use, int max)
{
  EmuAConvWide *c = (EmuAConvWide *) h;
  for (int co = 0; co < c->plan.s.out_ch && co < max; co++)
    use[co] = c->plan.use[(size_t) co];
  return c->plan.s.sparse;
}

void emu_aconv_wide_reset (void *h)
{
  EmuAConvWide *c = (EmuAConvWide *) h;
  std::fill (c->hist.begin (), c->hist.end (), 0);
  if (c->resampler) {
    emu_audio_free (c->resampler);
    c->resampler = wide_new_resampler (c, nullptr, 0);
  }
}

// in[] / out[]: one pointer for an interleaved side, `channels` for a non-interleaved one
void emu_aconv_wide_samples_planes (void *h, uint8_t *const *in, size_t in_frames, uint8_t *const *out, size_t out_frames)
{
  wide_run ((EmuAConvWide *) h, in, in_frames, out, out_frames);
}

// a non-interleaved side holds its channels one after the other
void emu_aconv_wide_samples (void *h, uint8_t *in, size_t in_frames, uint8_t *out, size_t out_frames)
{
  EmuAConvWide *c = (EmuAConvWide *) h;
  const AConvPlan &p = c->plan.s;
  uint8_t *ip[GSTAMD_AUDIO_MAX_CHANNELS_WIDE] = { nullptr }, *op[GSTAMD_AUDIO_MAX_CHANNELS_WIDE] = { nullptr };
  const size_t in_plane = in_frames * (size_t) afmt_bytes (p.in_fmt), out_plane = out_frames * (size_t) afmt_bytes (p.out_fmt);
  for (int k = 0; in && k < (c->in_layout ? p.in_ch : 1); k++)
    ip[k] = in + (size_t) k * in_plane;
  for (int k = 0; k < (c->out_layout ? p.out_ch : 1); k++)
    op[k] = out + (size_t) k * out_plane;
  wide_run (c, in ? ip : nullptr, in_frames, op, out_frames);
}

}  // extern "C"
