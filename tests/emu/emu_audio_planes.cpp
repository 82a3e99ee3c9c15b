// tests/emu/emu_audio_planes.cpp - TEST INFRASTRUCTURE: the audio converter with non-interleaved sides on the host the way the device
// runs it - the plan of aconv_make_plan_layouts, a loop over the rows and LANES of each launch (audio_convert_device.h aconv_pre_lane_planes /
// _pre_lane_mix / _post_lane_planes / aconv_shape_planes for a non-interleaved side, aconv_pre_lane / _post_lane / aconv_shape_channel for an interleaved
// one), block by block for the passthrough and the endian plan.  Mirrors aconv_run of audio_convert.hip; emu_audio_lanes.cpp is the
// interleaved-only twin (prefix "emu_aconv_lanes_"), this one's prefix is "emu_aconv_planes_".
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

static void *planes_new_resampler (EmuAConvPlanes *c, char *err, int err_len)
{
  GstAmdAudioResamplerOptions ro;
  if (c->cfg.has_resampler_options)
    ro = c->cfg.resampler_options;
  else
    audio_options_init (&ro);
  int st = 0;
  return emu_audio_new (c->cfg.resampler_method, (c->flags & 2) ? 4 : 0, c->plan.mid_in, c->out.channels, c->in.rate, c->out.rate, &ro, &st, err, err_len);
}

static bool planes_contiguous (uint8_t *const *pl, int n, size_t plane_bytes)
{
  for (int c = 1; c < n; c++)
    if (pl[c] != pl[c - 1] + plane_bytes)
      return false;
  return true;
}

static void planes_run (EmuAConvPlanes *c, uint8_t *const *in, size_t in_frames, uint8_t *const *out, size_t out_frames)
{
  const AConvPlan &p = c->plan;
  const size_t in_b = (size_t) afmt_bytes (p.in_fmt), out_b = (size_t) afmt_bytes (p.out_fmt);
  if (in_frames == 0)
    return;
  if (c->passthrough || p.endian_swap) {
    int blocks = c->out_layout ? p.out_ch : 1;
    size_t n = out_frames * (size_t) (c->out_layout ? 1 : p.out_ch);
    if (blocks > 1 && planes_contiguous (in, blocks, n * in_b) && planes_contiguous (out, blocks, n * out_b)) {
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
  if (in && c->in_layout) {              /* k_aconv_pre_planes: blockIdx.y = co */
    AConvPlanes src;
    memset (&src, 0, sizeof (src));
    for (int ci = 0; ci < p.in_ch; ci++)
      src.p[ci] = in[ci];
    src.frames = in_frames;
    aconv_planes_heads (&src, p.in_ch, p.out_ch, (int) in_b, aconv_pre_grouped_planes (p), !p.mix);
    const size_t lanes = aconv_planes_lanes (src, p.out_ch);
#define PRE(K) for (int co = 0; co < p.out_ch; co++) for (size_t t = 0; t < ((lanes + 255) / 256) * 256; t++) aconv_pre_lane_planes<K> (p, src, ma, co, t)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  } else if (in && c->out_layout && aconv_pre_grouped_mix (p)) {          /* k_aconv_pre_mix: blockIdx.y = co */
    const AConvSplit s = aconv_split (in[0], (int) in_b * p.in_ch, in_frames, true);
#define PRE(K) for (int co = 0; co < p.out_ch; co++) for (size_t t = 0; t < ((aconv_split_lanes (s) + 255) / 256) * 256; t++) aconv_pre_lane_mix<K> (p, in[0], ma, s, co, t)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  } else if (in) {                       /* k_aconv_pre */
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
  if (c->out_layout) {                   /* k_aconv_post_planes, k_aconv_shape_planes */
    AConvPlanes dst;
    memset (&dst, 0, sizeof (dst));
    for (int co = 0; co < p.out_ch; co++)
      dst.p[co] = out[co];
    dst.frames = out_frames;
    aconv_planes_heads (&dst, p.out_ch, p.out_ch, (int) out_b, aconv_post_grouped (p), true);
    const size_t lanes = aconv_planes_lanes (dst, p.out_ch);
#define POST(K) for (int co = 0; co < p.out_ch; co++) for (size_t t = 0; t < ((lanes + 255) / 256) * 256; t++) \
    aconv_post_lane_planes<K> (p, c->jump, c->dither, after, dst, qv.data (), qd.data (), co, t)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
    if (shape) {
#define SHAPE(K) aconv_shape_planes<K> (p, qv.data (), qd.data (), c->hist.data (), dst)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
    }
  } else {                               /* k_aconv_post, k_aconv_shape */
    const AConvSplit s = aconv_split (out[0], (int) out_b, samples, aconv_post_grouped (p));
#define POST(K) for (size_t t = 0; t < aconv_split_lanes (s); t++) aconv_post_lane<K> (p, c->jump, c->dither, after, out[0], qv.data (), qd.data (), s, t)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
    if (shape) {
#define SHAPE(K) for (int ch = 0; ch < p.out_ch; ch++) aconv_shape_channel<K> (p, qv.data (), qd.data (), c->hist.data (), out[0], out_frames, ch)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
    }
  }
  aconv_dither_advance (p, c->jump, &c->dither, samples);
}

extern "C" {

void *emu_aconv_planes_new (int flags, const GstAmdAudioInfo *in, int in_layout, const GstAmdAudioInfo *out, int out_layout, const GstAmdAudioConverterConfig *cfg,
    char *err, int err_len)
{
  EmuAConvPlanes *c = new EmuAConvPlanes ();
  std::string e;
  c->flags = flags;
  c->in_layout = in_layout;
  c->out_layout = out_layout;
  c->in = *in;
  c->out = *out;
  c->cfg = *cfg;
  if (aconv_make_plan_layouts (flags, in, in_layout, out, out_layout, *cfg, &c->plan, &c->resample, &c->passthrough, &e) != GSTAMD_OK) {
    if (err)
      strncpy (err, e.c_str (), err_len - 1);
    delete c;
    return nullptr;
  }
  if (c->resample && !(c->resampler = planes_new_resampler (c, err, err_len))) {
    delete c;
    return nullptr;
  }
  aconv_make_jump (&c->jump);
  return c;
}

void emu_aconv_planes_free (void *h)
{
  EmuAConvPlanes *c = (EmuAConvPlanes *) h;
  if (c && c->resampler)
    emu_audio_free (c->resampler);
  delete c;
}

size_t emu_aconv_planes_get_out_frames (void *h, size_t in_frames)
{
  EmuAConvPlanes *c = (EmuAConvPlanes *) h;
  return c->resampler ? emu_audio_get_out_frames (c->resampler, in_frames) : in_frames;
}

int emu_aconv_planes_is_passthrough (void *h) { return ((EmuAConvPlanes *) h)->passthrough ? 1 : 0; }

// gst_audio_converter_reset: the error history goes, the generator stays; the emulated resampler has no reset of its own, and a new
// one is what a reset one is (no update has touched it)
void emu_aconv_planes_reset (void *h)
{
  EmuAConvPlanes *c = (EmuAConvPlanes *) h;
  std::fill (c->hist.begin (), c->hist.end (), 0);
  if (c->resampler) {
    emu_audio_free (c->resampler);
    c->resampler = planes_new_resampler (c, nullptr, 0);
  }
}

// in[] / out[]: one pointer for an interleaved side, `channels` for a non-interleaved one
void emu_aconv_planes_samples_planes (void *h, uint8_t *const *in, size_t in_frames, uint8_t *const *out, size_t out_frames)
{
  planes_run ((EmuAConvPlanes *) h, in, in_frames, out, out_frames);
}

// a non-interleaved side holds its channels one after the other
void emu_aconv_planes_samples (void *h, uint8_t *in, size_t in_frames, uint8_t *out, size_t out_frames)
{
  EmuAConvPlanes *c = (EmuAConvPlanes *) h;
  uint8_t *ip[GSTAMD_AUDIO_MAX_CHANNELS] = { nullptr }, *op[GSTAMD_AUDIO_MAX_CHANNELS] = { nullptr };
  const size_t in_plane = in_frames * (size_t) afmt_bytes (c->plan.in_fmt), out_plane = out_frames * (size_t) afmt_bytes (c->plan.out_fmt);
  for (int k = 0; in && k < (c->in_layout ? c->plan.in_ch : 1); k++)
    ip[k] = in + (size_t) k * in_plane;
  for (int k = 0; k < (c->out_layout ? c->plan.out_ch : 1); k++)
    op[k] = out + (size_t) k * out_plane;
  planes_run (c, in ? ip : nullptr, in_frames, op, out_frames);
}

}  // extern "C"
