// tests/emu/emu_audio_many.cpp - TEST INFRASTRUCTURE: gstamd_audio_converter_samples_many on the host the way the device
// runs it - the same walk over the call's streams (aconv_many_run_length of audio_convert_plan.h), and for every batched run a loop over
// the grid of each launch: blockIdx.y = stream, blockIdx.x up to the longest stream's blocks, 256 lanes, through the bodies the kernels
// call (audio_convert_device.h aconv_pre_many_lane / _post_many_lane / _shape_many_lane) with the tables aconv_many_pre_entry /
// _post_entry fill.  Mirrors gstamd_audio_converter_samples_many / aconv_run_many of audio_convert.hip.
//
// The converters are the emulator's existing handles: those of emu_aconv_planes_new (emu_audio_planes.cpp: every converter of at most 8
// channels - interleaved, non-interleaved, passthrough, endian) and of emu_aconv_wide_new (emu_audio_wide.cpp), which the caller tells
// apart in kind[].  A stream that is not batched goes through its own emulator's emu_aconv_*_samples.
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
int emu_aconv_wide_is_passthrough (void *h);
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

enum { KIND_PLANES = 0, KIND_WIDE = 1, KIND_WIDE_RESAMPLER = 3 };

thread_local int32_t many_debug[4] = { 0, 0, 0, 0 };
const AConvPlan no_plan = {};                   // what a wide handle shows the decision: never looked at, `ordinary` is false

// a stream as aconv_many_run_length sees it
AConvManyItem item_of (void *h, int kind, bool has_input, size_t in_frames, size_t out_frames)
{
  if (kind & 1)
    return { &no_plan, h, false, kind == KIND_WIDE_RESAMPLER, has_input, in_frames, out_frames };
  const EmuAConvPlanes *c = (const EmuAConvPlanes *) h;
  return { &c->plan, c, !c->in_layout && !c->out_layout && !c->passthrough, c->resampler != nullptr, has_input, in_frames, out_frames };
}

// aconv_run_many
void many_run (int run, EmuAConvPlanes *const *cs, const uint8_t *const *in, const size_t *in_frames, uint8_t *const *out, const size_t *out_frames)
{
  const AConvPlan &p = cs[0]->plan;
  const size_t mb = (size_t) amid_bytes (p.mid_in) * (size_t) p.out_ch;
  const bool shape = aconv_plan_shapes (p), resample = cs[0]->resampler != nullptr;
  std::vector<std::vector<uint8_t>> mid_a ((size_t) run), mid_b ((size_t) run);
  std::vector<std::vector<int32_t>> q ((size_t) run);
  for (int k = 0; k < run; k++) {
    mid_a[(size_t) k].assign (in_frames[k] * mb, 0xcd);
    mid_b[(size_t) k].assign ((out_frames[k] ? out_frames[k] : 1) * mb, 0xcd);
    if (shape && out_frames[k])
      q[(size_t) k].assign (out_frames[k] * (size_t) p.out_ch * 2, 0);
  }
  {                                             /* k_aconv_pre_many */
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
    many_debug[3]++;
  }
  if (resample)                                 /* gstamd_audio_resampler_resample_many: independent streams, whatever the launch */
    for (int k = 0; k < run; k++)
      emu_audio_resample (cs[k]->resampler, mid_a[(size_t) k].data (), in_frames[k], mid_b[(size_t) k].data (), out_frames[k]);
  AConvManyPostTable t;
  AConvManyShapeTable sh;
  memset ((void *) &t, 0, sizeof (t));
  memset ((void *) &sh, 0, sizeof (sh));
  size_t lanes = 0;
  for (int k = 0; k < run; k++) {
    int32_t *qk = shape && out_frames[k] ? q[(size_t) k].data () : nullptr;
    const size_t l = aconv_many_post_entry (p, cs[k]->dither, resample ? mid_b[(size_t) k].data () : mid_a[(size_t) k].data (), out[k], out_frames[k], qk, &t.s[k]);
    lanes = l > lanes ? l : lanes;
    sh.s[k] = { qk, cs[k]->hist.data (), out[k], out_frames[k] };
  }
  if (lanes) {
    const size_t grid = ((lanes + 255) / 256) * 256;
#define POST(K) for (int y = 0; y < run; y++) for (size_t x = 0; x < grid; x++) aconv_post_many_lane<K> (p, cs[0]->jump, t.s[y], x)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);   /* k_aconv_post_many */
#undef POST
    many_debug[3]++;
    if (shape) {                                /* k_aconv_shape_many: blockIdx.x = stream, 64 lanes */
#define SHAPE(K) for (int y = 0; y < run; y++) for (int c = 0; c < 64; c++) aconv_shape_many_lane<K> (p, sh.s[y], c)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
      many_debug[3]++;
    }
  }
  for (int k = 0; k < run; k++)
    aconv_dither_advance (p, cs[k]->jump, &cs[k]->dither, out_frames[k] * (size_t) p.out_ch);
}

}  // namespace

extern "C" {

// gstamd_audio_converter_samples_many over emulator handles; kind[i]: 0 a handle of emu_aconv_planes_new, 1 of emu_aconv_wide_new, 3 the
// latter with a resampler inside (NULL: all 0).  Returns GSTAMD_OK or GSTAMD_ERR_INVALID, as the C ABI does.
int emu_aconv_many_samples (int n, void *const *handles, const int *kind, uint8_t *const *in, const size_t *in_frames, uint8_t *const *out, const size_t *out_frames)
{
  memset (many_debug, 0, sizeof (many_debug));
  if (n < 0 || (n > 0 && (!handles || !in_frames || !out_frames)))
    return GSTAMD_ERR_INVALID;
  auto wide = [&](int i) { return kind && (kind[i] & 1); };
  for (int i = 0; i < n; i++) {
    if (!handles[i] || (out_frames[i] && (!out || !out[i])))
      return GSTAMD_ERR_INVALID;
    if (in_frames[i] == 0)
      continue;
    const bool resampler = wide (i) ? kind[i] == KIND_WIDE_RESAMPLER : ((EmuAConvPlanes *) handles[i])->resampler != nullptr;
    const bool passthrough = wide (i) ? emu_aconv_wide_is_passthrough (handles[i]) != 0 : ((EmuAConvPlanes *) handles[i])->passthrough;
    if (!resampler && !(in && in[i]))
      return GSTAMD_ERR_INVALID;
    if (!resampler && !passthrough && in_frames[i] != out_frames[i])
      return GSTAMD_ERR_INVALID;
  }
  std::vector<AConvManyItem> items;
  std::vector<int> at;
  for (int i = 0; i < n; i++) {
    if (in_frames[i] == 0)
      continue;
    items.push_back (item_of (handles[i], kind ? kind[i] : 0, in && in[i] != nullptr, in_frames[i], out_frames[i]));
    at.push_back (i);
  }
  const int live = (int) items.size ();
  for (int done = 0; done < live;) {
    const int run = aconv_many_run_length (&items[(size_t) done], live - done);
    if (run < 2) {
      const int i = at[(size_t) done];
      (wide (i) ? emu_aconv_wide_samples : emu_aconv_planes_samples) (handles[i], in ? in[i] : nullptr, in_frames[i], out ? out[i] : nullptr, out_frames[i]);
      many_debug[2]++;
    } else {
      EmuAConvPlanes *cs[GSTAMD_ACONV_MANY_MAX];
      const uint8_t *ip[GSTAMD_ACONV_MANY_MAX];
      uint8_t *op[GSTAMD_ACONV_MANY_MAX];
      size_t inf[GSTAMD_ACONV_MANY_MAX], outf[GSTAMD_ACONV_MANY_MAX];
      for (int k = 0; k < run; k++) {
        const int i = at[(size_t) (done + k)];
        cs[k] = (EmuAConvPlanes *) handles[i];
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

int emu_aconv_many_debug (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = many_debug[i];
  return 4;
}

// aconv_many_run_length over the same handles, for a test that states the runs: the length of the run that starts at stream 0
int emu_aconv_many_run_length (int n, void *const *handles, const int *kind, uint8_t *const *in, const size_t *in_frames, const size_t *out_frames)
{
  std::vector<AConvManyItem> items;
  for (int i = 0; i < n; i++) {
    items.push_back (item_of (handles[i], kind ? kind[i] : 0, in && in[i] != nullptr, in_frames[i], out_frames[i]));
  }
  return aconv_many_run_length (items.data (), n);
}

}  // extern "C"
