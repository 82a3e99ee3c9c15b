// tests/emu/emu_audio_lanes.cpp - TEST INFRASTRUCTURE: the audio converter's kernels on the host the way the device runs them - a loop
// over the LANES of a launch (audio_convert_device.h aconv_pre_lane / _post_lane / _swap_lane: four samples on aligned dwords per lane,
// single samples at an unaligned head and tail), with the container chosen outside the loop as audio_convert.hip does, and the endian
// plan's swap kernel.  emu_audio.cpp's emu_aconv_* walks samples; this walks what k_aconv_pre / _post / _shape / _swap execute.
#include <cstring>
#include <string>
#include <vector>

#include "../../gstreamer_amd/csrc/audio_convert_plan.h"
#include "../../gstreamer_amd/csrc/audio_taps.h"

using namespace gstamd;

extern "C" {
void *emu_audio_new (int method, int flags, int format, int channels, int in_rate, int out_rate, const GstAmdAudioResamplerOptions *options, int *status, char *err,
    int err_len);
void emu_audio_free (void *h);
size_t emu_audio_get_out_frames (void *h, size_t in_frames);
void emu_audio_resample (void *h, const void *in, size_t in_frames, void *out, size_t out_frames);
}

struct EmuAConvLanes {
  AConvPlan plan;
  bool resample = false, passthrough = false;
  void *resampler = nullptr;
  AConvDitherState dither = { 0xc2d6038fu, 0u, 0 };
  AConvJump jump;
  std::vector<int32_t> hist = std::vector<int32_t> (8 * GSTAMD_AUDIO_MAX_CHANNELS, 0);
};

extern "C" {

void *emu_aconv_lanes_new (int flags, const GstAmdAudioInfo *in, const GstAmdAudioInfo *out, const GstAmdAudioConverterConfig *cfg, char *err, int err_len)
{
  EmuAConvLanes *c = new EmuAConvLanes ();
  std::string e;
  if (aconv_make_plan (flags, in, out, *cfg, &c->plan, &c->resample, &c->passthrough, &e) != GSTAMD_OK) {
    if (err)
      strncpy (err, e.c_str (), err_len - 1);
    delete c;
    return nullptr;
  }
  if (c->resample) {
    GstAmdAudioResamplerOptions ro;
    if (cfg->has_resampler_options)
      ro = cfg->resampler_options;
    else
      audio_options_init (&ro);
    int st = 0;
    c->resampler = emu_audio_new (cfg->resampler_method, (flags & 2) ? 4 : 0, c->plan.mid_in, out->channels, in->rate, out->rate, &ro, &st, err, err_len);
    if (!c->resampler) {
      delete c;
      return nullptr;
    }
  }
  aconv_make_jump (&c->jump);
  return c;
}

void emu_aconv_lanes_free (void *h)
{
  EmuAConvLanes *c = (EmuAConvLanes *) h;
  if (c && c->resampler)
    emu_audio_free (c->resampler);
  delete c;
}

size_t emu_aconv_lanes_get_out_frames (void *h, size_t in_frames)
{
  EmuAConvLanes *c = (EmuAConvLanes *) h;
  return c->resampler ? emu_audio_get_out_frames (c->resampler, in_frames) : in_frames;
}

int emu_aconv_lanes_is_passthrough (void *h) { return ((EmuAConvLanes *) h)->passthrough ? 1 : 0; }

void emu_aconv_lanes_samples (void *h, const uint8_t *in, size_t in_frames, uint8_t *out, size_t out_frames)
{
  EmuAConvLanes *c = (EmuAConvLanes *) h;
  const AConvPlan &p = c->plan;
  if (in_frames == 0)
    return;
  if (c->passthrough) {
    memcpy (out, in, out_frames * (size_t) p.out_ch * (size_t) afmt_bytes (p.out_fmt));
    return;
  }
  if (p.endian_swap) {                   /* k_aconv_swap */
    const AConvSplit s = aconv_swap_split (in, out, p.endian_swap, out_frames * (size_t) p.out_ch);
    for (size_t t = 0; t < aconv_split_lanes (s); t++)
      switch (p.endian_swap) {
        case 2: aconv_swap_lane<AK_2LE> (in, out, s, t); break;
        case 3: aconv_swap_lane<AK_3LE> (in, out, s, t); break;
        case 4: aconv_swap_lane<AK_4LE> (in, out, s, t); break;
        default: aconv_swap_lane<AK_8LE> (in, out, s, t); break;
      }
    return;
  }
  const size_t mb = (size_t) amid_bytes (p.mid_in) * (size_t) p.out_ch;
  std::vector<uint8_t> a ((in_frames ? in_frames : 1) * mb), b ((out_frames ? out_frames : 1) * mb);
  uint8_t *ma = a.data (), *mbuf = b.data ();
  if (in) {                              /* k_aconv_pre */
    const AConvSplit s = aconv_split (in, afmt_bytes (p.in_fmt), in_frames * (size_t) p.out_ch, aconv_pre_grouped (p));
#define PRE(K) for (size_t t = 0; t < aconv_split_lanes (s); t++) aconv_pre_lane<K> (p, in, ma, s, t)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }
  const uint8_t *after = ma;
  if (c->resampler) {
    emu_audio_resample (c->resampler, in ? ma : nullptr, in_frames, mbuf, out_frames);
    after = mbuf;
  }
  const size_t samples = out_frames * (size_t) p.out_ch;
  std::vector<int32_t> qv (samples + 1), qd (samples + 1);
  const AConvSplit s = aconv_split (out, afmt_bytes (p.out_fmt), samples, aconv_post_grouped (p));      /* k_aconv_post */
#define POST(K) for (size_t t = 0; t < aconv_split_lanes (s); t++) aconv_post_lane<K> (p, c->jump, c->dither, after, out, qv.data (), qd.data (), s, t)
  GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
  if (p.ns && p.quant_shift > 0) {       /* k_aconv_shape */
#define SHAPE(K) for (int ch = 0; ch < p.out_ch; ch++) aconv_shape_channel<K> (p, qv.data (), qd.data (), c->hist.data (), out, out_frames, ch)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
  }
  aconv_dither_advance (p, c->jump, &c->dither, samples);
}

}  // extern "C"
