// audio_mix_device.h - audiomixer's sum of many streams into one buffer: the launch plan and the per-piece body of k_audio_mix (shared
// with the host emulator, tests/emu/emu_audio_mix.cpp; see audio_device.h).  DESIGN 3.9.
//
// Reference semantics (subprojects/gst-plugins-base/gst/audiomixer/):
//   gst_audio_mixer_aggregate_one_buffer   gstaudiomixer.c: mute / volume < G_MINDOUBLE skip the pad; volume == 1.0 -> audiomixer_orc_add_*,
//                                          else audiomixer_orc_add_volume_* with volume_i16 = (gint) (volume * 2048), volume_i32 = (gint)
//                                          (volume * 134217728)
//   audiomixer_orc_add_s16 / _s32 / _f32 / _f64, _add_volume_*   gstaudiomixerorc.orc, as their C backups compute (saturating adds,
//                                          mulswl >> 11 / mulslq >> 27 with a saturating narrow, floats flushed by ORC_DENORMAL around every
//                                          operation)
// The reference clears the output and makes one read-modify-write pass over it per pad.  Here a lane owns an aligned 16-byte piece of the
// output, walks the pads in their order with the running sums in registers, and stores the piece once.
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gstamd_audio.h"
#include "../../include/gstamd_video.h"
#include "audio_convert_device.h"

#ifdef __HIPCC__
#define GSTAMD_AD __device__ __forceinline__
#else
#define GSTAMD_AD inline
#endif

namespace gstamd {

enum { AMIX_MAX_INPUTS = 64,    // descriptors in the arguments of one launch
  AMIX_LANES = 256,             // lanes of a workgroup, a piece each
  AMIX_MAX_BLOCKS = 2048,       // longer buffers: grid-stride
  AMIX_PIECE = 16,              // bytes of output a lane owns
  AMIX_BATCH = 4                // inputs whose loads are requested before the first of their adds (8 measured the same on an MI355X)
};

// one live input of a launch, 32 bytes
struct AMixIn {
  const void *data;             // first sample that lands in the output
  uint32_t out_offset, frames;  // in frames (the call refuses 2^30 frames and more)
  uint64_t vol;                 // S16 / S32: the integer volume; F32: the bits of fl ((float) volume) in the low word; F64: the bits of fl64 (volume)
  int32_t reserved;
  int32_t load_bytes;           // 16, 8, 4 or 2: the widest load every whole piece of this input can be read with (amix_load_bytes)
};

struct AMixArgs {
  void *out;
  uint64_t samples;             // out_frames * channels
  int32_t channels;
  int32_t n;                    // live inputs of this launch
  int32_t accumulate;           // 0: the sums start at zero; 1: at what the launch before left in `out` (more than 64 live inputs)
  int32_t lead;                 // samples between the 16-byte boundary at or before `out` and `out`: piece q holds samples q * NP - lead ..
  AMixIn in[AMIX_MAX_INPUTS];
};

// ---- the launch plan: library and emulator decide with these ---------------------------------------------------------------------------
inline int amix_sample_bytes (int format)
{
  switch (format) {
    case GSTAMD_AFMT_S16LE: return 2;
    case GSTAMD_AFMT_S32LE: case GSTAMD_AFMT_F32LE: return 4;
    case GSTAMD_AFMT_F64LE: return 8;
    default: return 0;
  }
}

// gst_audio_mixer_aggregate_one_buffer's test, and the inputs that bring nothing
inline bool amix_live (const GstAmdAudioMixerInput &in)
{
  return !in.mute && !(in.volume < DBL_MIN) && in.frames != 0 && in.data != nullptr;
}

// everything the call refuses, before any launch
inline int amix_check (int format, int channels, const GstAmdAudioMixerInput *inputs, int n_inputs, const void *out, size_t out_frames)
{
  if (format < GSTAMD_AFMT_S8 || format > GSTAMD_AFMT_F64BE)
    return GSTAMD_ERR_INVALID;
  const int bps = amix_sample_bytes (format);
  if (!bps)
    return GSTAMD_ERR_UNSUPPORTED;
  if (channels < 1 || channels > GSTAMD_AUDIO_MAX_CHANNELS_WIDE || n_inputs < 0 || (n_inputs > 0 && !inputs))
    return GSTAMD_ERR_INVALID;
  if (out_frames >= ((size_t) 1 << 30) || (!out && out_frames > 0) || ((uintptr_t) out % (uintptr_t) bps) != 0)
    return GSTAMD_ERR_INVALID;
  for (int i = 0; i < n_inputs; i++) {
    const GstAmdAudioMixerInput &in = inputs[i];
    if (((uintptr_t) in.data % (uintptr_t) bps) != 0)
      return GSTAMD_ERR_INVALID;
    if (in.out_offset > out_frames || in.frames > out_frames - in.out_offset)
      return GSTAMD_ERR_INVALID;
    if (!(in.volume >= 0.0 && in.volume <= 10.0))       /* NaN fails both */
      return GSTAMD_ERR_INVALID;
  }
  return GSTAMD_OK;
}

// Input alignment: a whole piece starts on a 16-byte boundary of the OUTPUT; the input sample under its first sample sits at
// data + (piece_first_sample - out_offset * channels) * bps, which is this many bytes past a 16-byte boundary for every whole piece alike
inline int amix_load_bytes (const void *out, const void *data, uint64_t first_sample, int bps)
{
  const uint64_t rel = ((uint64_t) (uintptr_t) data - first_sample * (uint64_t) bps - (uint64_t) (uintptr_t) out) & 15u;
  return rel == 0 ? 16 : (rel % 8 == 0 ? 8 : (rel % 4 == 0 ? 4 : 2));
}

inline uint64_t amix_volume_word (int format, double volume)
{
  switch (format) {
    case GSTAMD_AFMT_S16LE: return (uint64_t) (uint32_t) (int32_t) (volume * 2048.0);
    case GSTAMD_AFMT_S32LE: return (uint64_t) (uint32_t) (int32_t) (volume * 134217728.0);
    case GSTAMD_AFMT_F32LE: return orc_denormal_f (f_bits ((float) volume));
    default: return orc_denormal_d (d_bits (volume));
  }
}

GSTAMD_AC uint64_t amix_pieces (uint64_t samples, int lead, int bps)
{
  const uint64_t np = (uint64_t) (AMIX_PIECE / bps);
  return (samples + (uint64_t) lead + np - 1) / np;
}

inline unsigned amix_grid (uint64_t pieces)
{
  const uint64_t blocks = (pieces + AMIX_LANES - 1) / AMIX_LANES;
  return (unsigned) (blocks > AMIX_MAX_BLOCKS ? AMIX_MAX_BLOCKS : (blocks ? blocks : 1));
}

// The whole call: the live inputs in their order, in groups of 64, a launch each - the first starts its sums at zero, every further one at the
// output of the one before (the running sum is sequential, so the chain is exact).  No live input: one launch that writes silence.
// launch (const AMixArgs &, unsigned grid) -> false when it failed.  record: { launches, inputs mixed, inputs skipped, 0 }.
template <typename Launch>
inline int amix_run (int format, int channels, const GstAmdAudioMixerInput *inputs, int n_inputs, void *out, size_t out_frames, int32_t record[4],
    Launch launch)
{
  record[0] = record[1] = record[2] = record[3] = 0;
  const int status = amix_check (format, channels, inputs, n_inputs, out, out_frames);
  if (status != GSTAMD_OK)
    return status;
  for (int i = 0; i < n_inputs; i++)
    record[amix_live (inputs[i]) ? 1 : 2]++;
  if (out_frames == 0)
    return GSTAMD_OK;
  const int bps = amix_sample_bytes (format);
  AMixArgs a;
  memset ((void *) &a, 0, sizeof (a));
  a.out = out;
  a.samples = (uint64_t) out_frames * (uint64_t) channels;
  a.channels = channels;
  a.lead = (int32_t) (((uintptr_t) out & 15u) / (uintptr_t) bps);
  const unsigned grid = amix_grid (amix_pieces (a.samples, a.lead, bps));
  for (int i = 0;;) {
    a.n = 0;
    for (; i < n_inputs && a.n < AMIX_MAX_INPUTS; i++) {
      if (!amix_live (inputs[i]))
        continue;
      AMixIn &d = a.in[a.n++];
      d.data = inputs[i].data;
      d.out_offset = (uint32_t) inputs[i].out_offset;
      d.frames = (uint32_t) inputs[i].frames;
      d.vol = amix_volume_word (format, inputs[i].volume);
      d.load_bytes = amix_load_bytes (out, d.data, (uint64_t) d.out_offset * (uint64_t) channels, bps);
    }
    if (!launch (a, grid))
      return GSTAMD_ERR_HIP;
    record[0]++;
    for (; i < n_inputs && !amix_live (inputs[i]); i++) ;
    if (i >= n_inputs)
      return GSTAMD_OK;
    a.accumulate = 1;
  }
}

// ---- the body ----------------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif

// a value that is the same in every lane, kept in a scalar register: the descriptors are then read by scalar loads from the arguments
#ifdef __HIP_DEVICE_COMPILE__
#define GSTAMD_AMIX_UNIFORM(x) __builtin_amdgcn_readfirstlane (x)
#define GSTAMD_AMIX_LOADS_FIRST() __builtin_amdgcn_sched_barrier (0)    /* no add is scheduled in between the loads of a batch */
#else
#define GSTAMD_AMIX_UNIFORM(x) (x)
#define GSTAMD_AMIX_LOADS_FIRST() ((void) 0)
#endif

struct __attribute__ ((may_alias, aligned (16))) AMixV16 { uint32_t w[4]; };
struct __attribute__ ((may_alias, aligned (8))) AMixV8 { uint32_t w[2]; };
struct __attribute__ ((may_alias, aligned (4))) AMixV4 { uint32_t w[1]; };
struct __attribute__ ((may_alias, aligned (2))) AMixV2 { uint16_t w[1]; };

// One sample of one input onto the running sum (the table of DESIGN 3.9.1).  The reference adds a pad of volume 1.0 without scaling it; here
// every sample is scaled, because scaling by 1.0 is the identity in each format: (s * 2048) >> 11 and ((int64) s * 2^27) >> 27 are s, inside
// the clamp's range, and fl (fl (s) * 1.0) is fl (s) for every s that is not a NaN (whose payload is not pinned).  One path, no branch per
// input.
GSTAMD_AD int16_t amix_add (int16_t d, int16_t s, const AMixIn &in)
{
  int32_t t = ((int32_t) s * (int32_t) (uint32_t) in.vol) >> 11;
  t = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
  t += d;
  return (int16_t) (t < -32768 ? -32768 : (t > 32767 ? 32767 : t));
}

GSTAMD_AD int32_t amix_add (int32_t d, int32_t s, const AMixIn &in)
{
  const int64_t lo = -((int64_t) 1 << 31), hi = ((int64_t) 1 << 31) - 1;
  int64_t t = ((int64_t) s * (int64_t) (int32_t) (uint32_t) in.vol) >> 27;
  t = t < lo ? lo : (t > hi ? hi : t);
  t += d;
  return (int32_t) (t < lo ? lo : (t > hi ? hi : t));
}

// (fl (d) of the table is d itself: a running sum is zero, the flushed result of the add before, or - in a further launch - such a result read
// back from the output)
GSTAMD_AD float amix_add (float d, float s, const AMixIn &in)
{
  const uint32_t t = orc_denormal_f (f_bits (bits_f (orc_denormal_f (f_bits (s))) * bits_f ((uint32_t) in.vol)));
  return bits_f (orc_denormal_f (f_bits (d + bits_f (t))));
}

GSTAMD_AD double amix_add (double d, double s, const AMixIn &in)
{
  const uint64_t t = orc_denormal_d (d_bits (bits_d (orc_denormal_d (d_bits (s))) * bits_d (in.vol)));
  return bits_d (orc_denormal_d (d_bits (d + bits_d (t))));
}

// The 16 bytes of input `in` (which starts at output sample i0) under the whole piece that starts at output sample p0, the input covering
// all of it: loads of in.load_bytes, the same choice in every lane
template <typename T>
GSTAMD_AD void amix_load_whole (const AMixIn &in, uint64_t i0, int64_t p0, T *s)
{
  const uint8_t *src = (const uint8_t *) ((const T *) in.data + ((uint64_t) p0 - i0));
  uint32_t w[4];
  if (in.load_bytes == 16) {
    const AMixV16 v = *(const AMixV16 *) src;
    for (int e = 0; e < 4; e++)
      w[e] = v.w[e];
  } else if (in.load_bytes == 8) {
    const AMixV8 v0 = ((const AMixV8 *) src)[0], v1 = ((const AMixV8 *) src)[1];
    w[0] = v0.w[0], w[1] = v0.w[1], w[2] = v1.w[0], w[3] = v1.w[1];
  } else if (sizeof (T) != 2 || in.load_bytes == 4) {
    for (int e = 0; e < 4; e++)
      w[e] = ((const AMixV4 *) src)[e].w[0];
  } else {
    for (int e = 0; e < 4; e++)
      w[e] = (uint32_t) ((const AMixV2 *) src)[2 * e].w[0] | ((uint32_t) ((const AMixV2 *) src)[2 * e + 1].w[0] << 16);
  }
  memcpy (s, w, 16);
}

// The same for a piece at an edge - of the output, or of the input's window: sample by sample, inside both; bit e of the result is set
// for every sample the input has there
template <typename T>
GSTAMD_AD uint32_t amix_load_part (const AMixIn &in, uint64_t i0, uint64_t i1, int64_t p0, uint64_t samples, T *s)
{
  constexpr int NP = AMIX_PIECE / (int) sizeof (T);
  const T *data = (const T *) in.data;
  uint32_t m = 0;
  for (int e = 0; e < NP; e++) {
    const int64_t idx = p0 + e;
    s[e] = (T) 0;
    if (idx >= 0 && (uint64_t) idx < samples && (uint64_t) idx >= i0 && (uint64_t) idx < i1) {
      s[e] = data[(uint64_t) idx - i0];
      m |= 1u << e;
    }
  }
  return m;
}

// Lane `lane` of the workgroup whose first piece is q0.  What depends on the arguments and q0 alone is the same in every lane of the
// workgroup: the walk over the inputs, the test that leaves out an input with nothing under the workgroup's 256 pieces, and the choice
// between whole loads (every piece of the workgroup inside the output, the input under all of them) and the sample-by-sample merge.
// Where the next AMIX_BATCH inputs all take whole loads, their loads are requested together, ahead of the first of their adds.
template <typename T>
GSTAMD_AD void amix_lane (const AMixArgs &a, uint64_t q0, int lane)
{
  constexpr int NP = AMIX_PIECE / (int) sizeof (T);
  const uint64_t samples = a.samples, channels = (uint64_t) a.channels;
  const int64_t w0 = (int64_t) (q0 * NP) - a.lead, w1 = w0 + (int64_t) AMIX_LANES * NP;   /* the workgroup's span of output samples */
  const bool inner = w0 >= 0 && (uint64_t) w1 <= samples;
  const uint64_t ws0 = w0 < 0 ? 0 : (uint64_t) w0, ws1 = (uint64_t) w1 < samples ? (uint64_t) w1 : samples;
  const int64_t p0 = w0 + (int64_t) lane * NP;                          /* the piece's first sample */
  if (p0 >= (int64_t) samples)
    return;
  const bool whole = p0 >= 0 && (uint64_t) p0 + NP <= samples;
  T *out = (T *) a.out;
  T d[NP];
  for (int e = 0; e < NP; e++)
    d[e] = (T) 0;
  if (a.accumulate) {
    if (whole) {
      const AMixV16 v = *(const AMixV16 *) (out + p0);
      memcpy (d, &v, 16);
    } else {
      for (int e = 0; e < NP; e++)
        if (p0 + e >= 0 && (uint64_t) (p0 + e) < samples)
          d[e] = out[p0 + e];
    }
  }
  for (int k = 0; k < a.n;) {
    const int ku = GSTAMD_AMIX_UNIFORM (k);
    k = ku;
    AMixIn in[AMIX_BATCH];                      /* the next descriptors, fetched together (past the last live one: zeros, not used) */
    for (int j = 0; j < AMIX_BATCH; j++)
      in[j] = a.in[k + j < AMIX_MAX_INPUTS ? k + j : AMIX_MAX_INPUTS - 1];
    int batch = (int) inner & (int) (k + AMIX_BATCH <= a.n);
    for (int j = 0; j < AMIX_BATCH; j++) {
      const uint64_t i0 = (uint64_t) in[j].out_offset * channels;
      batch &= (int) (i0 <= ws0) & (int) (i0 + (uint64_t) in[j].frames * channels >= ws1);
    }
    if (GSTAMD_AMIX_UNIFORM (batch)) {
      T s[AMIX_BATCH][NP];
      for (int j = 0; j < AMIX_BATCH; j++)
        amix_load_whole<T> (in[j], (uint64_t) in[j].out_offset * channels, p0, s[j]);
      GSTAMD_AMIX_LOADS_FIRST ();
      for (int j = 0; j < AMIX_BATCH; j++)
        for (int e = 0; e < NP; e++)
          d[e] = amix_add (d[e], s[j][e], in[j]);
      k += AMIX_BATCH;
      continue;
    }
    k++;
    const uint64_t i0 = (uint64_t) in[0].out_offset * channels, i1 = i0 + (uint64_t) in[0].frames * channels;
    if (i0 >= ws1 || i1 <= ws0)
      continue;
    T s[NP];
    if (inner && i0 <= ws0 && i1 >= ws1) {
      amix_load_whole<T> (in[0], i0, p0, s);
      for (int e = 0; e < NP; e++)
        d[e] = amix_add (d[e], s[e], in[0]);
    } else {
      const uint32_t m = amix_load_part<T> (in[0], i0, i1, p0, samples, s);
      for (int e = 0; e < NP; e++)
        if (m & (1u << e))
          d[e] = amix_add (d[e], s[e], in[0]);
    }
  }
  if (whole) {
    AMixV16 v;
    memcpy (&v, d, 16);
    *(AMixV16 *) (out + p0) = v;
  } else {
    for (int e = 0; e < NP; e++)
      if (p0 + e >= 0 && (uint64_t) (p0 + e) < samples)
        out[p0 + e] = d[e];
  }
}

}  // namespace gstamd
