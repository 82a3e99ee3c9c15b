// audio_volume_device.h - the volume element's sample loops on many buffers a launch: the launch plan and the per-piece body of
// k_audio_volume (shared with the host emulator, tests/emu/emu_audio_volume.cpp; see audio_device.h).  DESIGN 3.10.
//
// Reference semantics (subprojects/gst-plugins-base/gst/volume/):
//   volume_update_volume              gstvolume.c: the volume is held as a gfloat; mute or 0.0 -> silence, (gint) (volume * 2048) == 2048 ->
//                                     passthrough, else volume_i8 / _i16 / _i24 / _i32 = (gint) (volume * 8 / 2048 / 524288 / 134217728)
//   volume_process_int8 .. _int32, _float, _double and their _clamp forms        gstvolume.c, volume_orc_process_* of gstvolumeorc.orc
//   volume_process_controlled_*       gstvolume.c: 1 and 2 channels through volume_orc_process_controlled_*_1ch / _2ch (float arithmetic for
//                                     int8 / int16 / f32, ORC's denormal flush), any other count through the plain C loops on doubles
//   volume_orc_prepare_volumes        gstvolumeorc.orc: mute turns every gain into +0.0
// Here a lane owns an aligned 16-byte piece of a buffer's output (S24: a group of four samples), reads the input under it, and stores it
// once; up to 64 buffers, of any of the four kinds, are the descriptors of one launch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gstamd_audio.h"
#include "../../include/gstamd_video.h"
#include "audio_convert_device.h"

#ifndef GSTAMD_AD
#ifdef __HIPCC__
#define GSTAMD_AD __device__ __forceinline__
#else
#define GSTAMD_AD inline
#endif
#endif

namespace gstamd {

enum { AVOL_MAX_BUFFERS = 64,   // descriptors in the arguments of one launch
  AVOL_LANES = 256,             // lanes of a workgroup, a piece each
  AVOL_MAX_BLOCKS = 2048,       // per buffer; longer buffers: grid-stride
  AVOL_PIECE = 16               // bytes of output a lane owns (S24: 12, four samples)
};

// what the kernel does with a buffer
enum AVolMode : int32_t { AVOL_COPY = 0,        // passthrough out of place
  AVOL_ZERO = 1,                // silence: nothing is read
  AVOL_SCALE = 2,               // rule (a)
  AVOL_GAINS = 3,               // rule (b)
  AVOL_GAINS_MUTE = 4           // rule (b) with every gain +0.0: the gains are not read
};

// the sample type of S24LE: three bytes, never loaded as such
struct AVolS24 { uint8_t b[3]; };

// one buffer of a launch, 48 bytes
struct AVolBuf {
  const void *in;
  void *out;
  const double *gains;
  uint64_t vol;                 // integers: the integer volume; F32: the bits of fl ((float) vf) in the low word; F64: the bits of fl64 (vf)
  uint32_t frames;              // the call refuses 2^30 frames and more
  int32_t mode;                 // AVolMode
  int32_t load_bytes;           // the widest load every whole piece of the input can be read with (avol_load_bytes); S24: 4 or 1
  int32_t reserved;
};

struct AVolArgs {
  int32_t channels;
  int32_t n;                    // descriptors of this launch: gridDim.y
  int32_t reserved[2];
  AVolBuf buf[AVOL_MAX_BUFFERS];
};

// ---- the launch plan: library and emulator decide with these ---------------------------------------------------------------------------
inline int avol_sample_bytes (int format)
{
  switch (format) {
    case GSTAMD_AFMT_S8: return 1;
    case GSTAMD_AFMT_S16LE: return 2;
    case GSTAMD_AFMT_S24LE: return 3;
    case GSTAMD_AFMT_S32LE: case GSTAMD_AFMT_F32LE: return 4;
    case GSTAMD_AFMT_F64LE: return 8;
    default: return 0;
  }
}

// volume_update_volume: the element's volume is a float
inline double avol_held (double volume) { return (double) (float) volume; }

// rule (a)'s three ways, in the reference's order
inline bool avol_silent (const GstAmdAudioVolumeBuffer &b) { return b.mute || avol_held (b.volume) == 0.0; }
inline bool avol_unity (const GstAmdAudioVolumeBuffer &b) { return !avol_silent (b) && (int) (avol_held (b.volume) * 2048.0) == 2048; }

inline int32_t avol_mode (const GstAmdAudioVolumeBuffer &b)
{
  if (b.gains)
    return b.mute ? AVOL_GAINS_MUTE : AVOL_GAINS;
  return avol_silent (b) ? AVOL_ZERO : (avol_unity (b) ? AVOL_COPY : AVOL_SCALE);
}

// a buffer that passes through in place needs nothing
inline bool avol_needs_kernel (const GstAmdAudioVolumeBuffer &b)
{
  return b.frames != 0 && !(avol_mode (b) == AVOL_COPY && b.in == b.out);
}

inline uint64_t avol_volume_word (int format, double volume)
{
  const double vf = avol_held (volume);
  switch (format) {
    case GSTAMD_AFMT_S8: return (uint64_t) (uint32_t) (int32_t) (vf * 8.0);
    case GSTAMD_AFMT_S16LE: return (uint64_t) (uint32_t) (int32_t) (vf * 2048.0);
    case GSTAMD_AFMT_S24LE: return (uint64_t) (uint32_t) (int32_t) (vf * 524288.0);
    case GSTAMD_AFMT_S32LE: return (uint64_t) (uint32_t) (int32_t) (vf * 134217728.0);
    case GSTAMD_AFMT_F32LE: return orc_denormal_f (f_bits ((float) vf));
    default: return orc_denormal_d (d_bits (vf));
  }
}

// Input alignment: a whole piece starts on a 16-byte boundary of the OUTPUT, and the input under it sits (in - out) mod 16 bytes past one, for
// every whole piece alike.  S24: the three dwords of a group are aligned where both pointers are
inline int avol_load_bytes (const void *out, const void *in, int bps)
{
  if (bps == 3)
    return ((((uintptr_t) in | (uintptr_t) out) & 3u) == 0) ? 4 : 1;
  const unsigned rel = (unsigned) (((uintptr_t) in - (uintptr_t) out) & 15u);
  return rel == 0 ? 16 : (rel % 8 == 0 ? 8 : (rel % 4 == 0 ? 4 : (rel % 2 == 0 ? 2 : 1)));
}

// samples between the 16-byte boundary at or before `out` and `out` (S24: pieces are counted from `out`)
GSTAMD_AC int avol_lead (const void *out, int bps) { return bps == 3 ? 0 : (int) (((uintptr_t) out & 15u) / (uintptr_t) bps); }

GSTAMD_AC uint64_t avol_pieces (uint64_t samples, int lead, int bps)
{
  const uint64_t np = bps == 3 ? 4u : (uint64_t) (AVOL_PIECE / bps);
  return (samples + (uint64_t) lead + np - 1) / np;
}

inline unsigned avol_grid (uint64_t pieces)
{
  const uint64_t blocks = (pieces + AVOL_LANES - 1) / AVOL_LANES;
  return (unsigned) (blocks > AVOL_MAX_BLOCKS ? AVOL_MAX_BLOCKS : (blocks ? blocks : 1));
}

// everything the call refuses, before any launch
inline int avol_check (int format, int channels, const GstAmdAudioVolumeBuffer *buffers, int n)
{
  if (format < GSTAMD_AFMT_S8 || format > GSTAMD_AFMT_F64BE)
    return GSTAMD_ERR_INVALID;
  const int bps = avol_sample_bytes (format);
  if (!bps)
    return GSTAMD_ERR_UNSUPPORTED;
  if (channels < 1 || channels > GSTAMD_AUDIO_MAX_CHANNELS_WIDE || n < 0 || (n > 0 && !buffers))
    return GSTAMD_ERR_INVALID;
  const uintptr_t align = bps == 3 ? 1u : (uintptr_t) bps;
  for (int i = 0; i < n; i++) {
    const GstAmdAudioVolumeBuffer &b = buffers[i];
    if (b.frames >= ((uint64_t) 1 << 30) || (b.frames > 0 && (!b.in || !b.out)))
      return GSTAMD_ERR_INVALID;
    if (((uintptr_t) b.in % align) != 0 || ((uintptr_t) b.out % align) != 0 || ((uintptr_t) b.gains % 8u) != 0)
      return GSTAMD_ERR_INVALID;
    const uintptr_t bytes = (uintptr_t) (b.frames * (uint64_t) channels * (uint64_t) bps), in = (uintptr_t) b.in, out = (uintptr_t) b.out;
    if (in != out && in < out + bytes && out < in + bytes)
      return GSTAMD_ERR_INVALID;
    if (!b.gains && !(b.volume >= 0.0 && b.volume <= 10.0))     /* NaN fails both */
      return GSTAMD_ERR_INVALID;
  }
  return GSTAMD_OK;
}

// The whole call: every buffer that needs the kernel is a descriptor, in array order, in groups of 64, a launch each; the grid's x is the
// longest buffer's of the group.  launch (const AVolArgs &, unsigned grid_x) -> false when it failed.
// record: { launches, buffers scaled (rule (a)'s formulas, or rule (b)), buffers passed through, buffers silenced }.
template <typename Launch>
inline int avol_run (int format, int channels, const GstAmdAudioVolumeBuffer *buffers, int n, int32_t record[4], Launch launch)
{
  record[0] = record[1] = record[2] = record[3] = 0;
  const int status = avol_check (format, channels, buffers, n);
  if (status != GSTAMD_OK)
    return status;
  const int bps = avol_sample_bytes (format);
  for (int i = 0; i < n; i++) {
    if (buffers[i].frames == 0)
      continue;
    const int32_t mode = avol_mode (buffers[i]);
    record[mode == AVOL_COPY ? 2 : (mode == AVOL_ZERO ? 3 : 1)]++;
  }
  AVolArgs a;
  memset ((void *) &a, 0, sizeof (a));
  a.channels = channels;
  for (int i = 0; i < n;) {
    unsigned grid = 0;
    a.n = 0;
    for (; i < n && a.n < AVOL_MAX_BUFFERS; i++) {
      const GstAmdAudioVolumeBuffer &b = buffers[i];
      if (!avol_needs_kernel (b))
        continue;
      AVolBuf &d = a.buf[a.n++];
      d.in = b.in;
      d.out = b.out;
      d.gains = b.gains;
      d.frames = (uint32_t) b.frames;
      d.mode = avol_mode (b);
      d.vol = d.mode == AVOL_SCALE ? avol_volume_word (format, b.volume) : 0;
      d.load_bytes = avol_load_bytes (b.out, b.in, bps);
      const unsigned g = avol_grid (avol_pieces (b.frames * (uint64_t) channels, avol_lead (b.out, bps), bps));
      grid = g > grid ? g : grid;
    }
    if (a.n == 0)
      break;
    if (!launch (a, grid))
      return GSTAMD_ERR_HIP;
    record[0]++;
  }
  return GSTAMD_OK;
}

// ---- the body ----------------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif

struct __attribute__ ((may_alias, aligned (16))) AVolV16 { uint32_t w[4]; };
struct __attribute__ ((may_alias, aligned (8))) AVolV8 { uint32_t w[2]; };
struct __attribute__ ((may_alias, aligned (4))) AVolV4 { uint32_t w[1]; };
struct __attribute__ ((may_alias, aligned (2))) AVolV2 { uint16_t w[1]; };

// sample <-> the bits it travels as
GSTAMD_AD int32_t avol_clamp (int64_t t, int bits)
{
  const int64_t lo = -((int64_t) 1 << (bits - 1)), hi = ((int64_t) 1 << (bits - 1)) - 1;
  return (int32_t) (t < lo ? lo : (t > hi ? hi : t));
}

// satN (trunc (t)): the clamp first, so that the cast is always inside the integer's range; a NaN gives 0 (not pinned)
GSTAMD_AD int32_t avol_trunc_f (float t, int bits)
{
  const float lo = -(float) ((int64_t) 1 << (bits - 1)), hi = (float) (((int64_t) 1 << (bits - 1)) - 1);
  return t != t ? 0 : (int32_t) (t < lo ? lo : (t > hi ? hi : t));
}

GSTAMD_AD int32_t avol_trunc_d (double t, int bits)
{
  const double lo = -(double) ((int64_t) 1 << (bits - 1)), hi = (double) (((int64_t) 1 << (bits - 1)) - 1);
  return t != t ? 0 : (int32_t) (t < lo ? lo : (t > hi ? hi : t));
}

// rule (a), one sample (the table of DESIGN 3.10.1)
GSTAMD_AD int8_t avol_scale (int8_t s, uint64_t vol) { return (int8_t) avol_clamp (((int32_t) s * (int32_t) (uint32_t) vol) >> 3, 8); }
GSTAMD_AD int16_t avol_scale (int16_t s, uint64_t vol) { return (int16_t) avol_clamp (((int32_t) s * (int32_t) (uint32_t) vol) >> 11, 16); }
GSTAMD_AD int32_t avol_scale24 (int32_t s, uint64_t vol) { return avol_clamp (((int64_t) s * (int64_t) (int32_t) (uint32_t) vol) >> 19, 24); }
GSTAMD_AD int32_t avol_scale (int32_t s, uint64_t vol) { return avol_clamp (((int64_t) s * (int64_t) (int32_t) (uint32_t) vol) >> 27, 32); }
GSTAMD_AD float avol_scale (float s, uint64_t vol)
{
  return bits_f (orc_denormal_f (f_bits (bits_f (orc_denormal_f (f_bits (s))) * bits_f ((uint32_t) vol))));
}
GSTAMD_AD double avol_scale (double s, uint64_t vol)
{
  return bits_d (orc_denormal_d (d_bits (bits_d (orc_denormal_d (d_bits (s))) * bits_d (vol))));
}

// rule (b), one sample with its frame's gain; wide: the reference's plain C loop on doubles (3 channels and more; F64: 2 and more; S24 and
// S32: always), else its ORC program
GSTAMD_AD float avol_gain_f (double g) { return bits_f (orc_denormal_f (f_bits ((float) g))); }
GSTAMD_AD int8_t avol_gain (int8_t s, double g, bool wide)
{
  if (wide)
    return (int8_t) avol_trunc_d ((double) s * g, 8);
  return (int8_t) avol_trunc_f (bits_f (orc_denormal_f (f_bits ((float) s * avol_gain_f (g)))), 8);
}
GSTAMD_AD int16_t avol_gain (int16_t s, double g, bool wide)
{
  if (wide)
    return (int16_t) avol_trunc_d ((double) s * g, 16);
  return (int16_t) avol_trunc_f (bits_f (orc_denormal_f (f_bits ((float) s * avol_gain_f (g)))), 16);
}
GSTAMD_AD int32_t avol_gain24 (int32_t s, double g) { return avol_trunc_d ((double) s * g, 24); }
GSTAMD_AD int32_t avol_gain (int32_t s, double g, bool) { return avol_trunc_d ((double) s * g, 32); }
GSTAMD_AD float avol_gain (float s, double g, bool wide)
{
  if (wide)
    return (float) ((double) s * g);            /* plain IEEE: denormals in, denormals out */
  return bits_f (orc_denormal_f (f_bits (bits_f (orc_denormal_f (f_bits (s))) * avol_gain_f (g))));
}
GSTAMD_AD double avol_gain (double s, double g, bool wide)
{
  if (wide)
    return s * g;                               /* plain IEEE */
  return bits_d (orc_denormal_d (d_bits (bits_d (orc_denormal_d (d_bits (s))) * bits_d (orc_denormal_d (d_bits (g))))));
}

template <typename T> GSTAMD_AD bool avol_wide (int channels) { return channels >= 3; }
template <> GSTAMD_AD bool avol_wide<int32_t> (int) { return true; }
template <> GSTAMD_AD bool avol_wide<double> (int channels) { return channels >= 2; }

// frame and channel of sample i: one division per piece, none where a frame is one or two samples
GSTAMD_AD void avol_frame_of (uint64_t i, uint32_t channels, uint32_t *frame, uint32_t *channel)
{
  if (channels == 1) {
    *frame = (uint32_t) i, *channel = 0;
  } else if (channels == 2) {
    *frame = (uint32_t) (i >> 1), *channel = (uint32_t) (i & 1u);
  } else {
    *frame = (uint32_t) (i / channels);
    *channel = (uint32_t) (i - (uint64_t) *frame * channels);
  }
}

// The 16 input bytes under a whole piece, with loads of load_bytes: the same choice in every lane of the buffer's workgroups
template <typename T>
GSTAMD_AD void avol_load_whole (const uint8_t *src, int load_bytes, T *s)
{
  uint32_t w[4];
  if (load_bytes == 16) {
    const AVolV16 v = *(const AVolV16 *) src;
    for (int e = 0; e < 4; e++)
      w[e] = v.w[e];
  } else if (load_bytes == 8) {
    const AVolV8 v0 = ((const AVolV8 *) src)[0], v1 = ((const AVolV8 *) src)[1];
    w[0] = v0.w[0], w[1] = v0.w[1], w[2] = v1.w[0], w[3] = v1.w[1];
  } else if (sizeof (T) == 4 || load_bytes == 4) {
    for (int e = 0; e < 4; e++)
      w[e] = ((const AVolV4 *) src)[e].w[0];
  } else if (sizeof (T) == 2 || load_bytes == 2) {
    for (int e = 0; e < 4; e++)
      w[e] = (uint32_t) ((const AVolV2 *) src)[2 * e].w[0] | ((uint32_t) ((const AVolV2 *) src)[2 * e + 1].w[0] << 16);
  } else {
    for (int e = 0; e < 4; e++)
      w[e] = (uint32_t) src[4 * e] | ((uint32_t) src[4 * e + 1] << 8) | ((uint32_t) src[4 * e + 2] << 16) | ((uint32_t) src[4 * e + 3] << 24);
  }
  memcpy (s, w, 16);
}

// Lane `lane` of a workgroup of buffer b whose first piece is q0: the input under the lane's piece is read whole before the piece is written,
// and no lane reads outside its own piece, so in == out is safe.  The mode, the load width and the channel rule are the same in every lane.
template <typename T>
GSTAMD_AD void avol_lane (const AVolBuf &b, int channels, uint64_t q0, int lane)
{
  constexpr int NP = AVOL_PIECE / (int) sizeof (T);
  const uint64_t samples = (uint64_t) b.frames * (uint64_t) channels;
  const int64_t p0 = (int64_t) ((q0 + (uint64_t) lane) * NP) - avol_lead (b.out, (int) sizeof (T));       /* the piece's first sample */
  if (p0 >= (int64_t) samples)
    return;
  const bool whole = p0 >= 0 && (uint64_t) p0 + NP <= samples;
  const T *in = (const T *) b.in;
  T *out = (T *) b.out;
  T s[NP], d[NP];
  for (int e = 0; e < NP; e++)
    s[e] = (T) 0;
  if (b.mode != AVOL_ZERO) {
    if (whole) {
      avol_load_whole<T> ((const uint8_t *) (in + p0), b.load_bytes, s);
    } else {
      for (int e = 0; e < NP; e++)
        if (p0 + e >= 0 && (uint64_t) (p0 + e) < samples)
          s[e] = in[p0 + e];
    }
  }
  if (b.mode == AVOL_SCALE) {
    for (int e = 0; e < NP; e++)
      d[e] = avol_scale (s[e], b.vol);
  } else if (b.mode == AVOL_GAINS || b.mode == AVOL_GAINS_MUTE) {
    const bool wide = avol_wide<T> (channels);
    uint32_t frame, channel;
    avol_frame_of (p0 < 0 ? 0 : (uint64_t) p0, (uint32_t) channels, &frame, &channel);
    for (int e = 0; e < NP; e++) {
      double g = 0.0;
      if (whole || (p0 + e >= 0 && (uint64_t) (p0 + e) < samples)) {
        if (b.mode == AVOL_GAINS)
          g = b.gains[frame];
        if (++channel == (uint32_t) channels)
          channel = 0, frame++;
      }
      d[e] = avol_gain (s[e], g, wide);
    }
  } else {                      /* a copy, or the zeros s holds */
    for (int e = 0; e < NP; e++)
      d[e] = s[e];
  }
  if (whole) {
    AVolV16 v;
    memcpy (&v, d, 16);
    *(AVolV16 *) (out + p0) = v;
  } else {
    for (int e = 0; e < NP; e++)
      if (p0 + e >= 0 && (uint64_t) (p0 + e) < samples)
        out[p0 + e] = d[e];
  }
}

// S24: a lane owns four samples = 12 bytes counted from `out`; three dword accesses where both pointers are 4-byte aligned, single bytes
// at any other alignment and in the last group of a buffer whose sample count is no multiple of four
template <>
GSTAMD_AD void avol_lane<AVolS24> (const AVolBuf &b, int channels, uint64_t q0, int lane)
{
  const uint64_t samples = (uint64_t) b.frames * (uint64_t) channels;
  const uint64_t p0 = (q0 + (uint64_t) lane) * 4u;
  if (p0 >= samples)
    return;
  const bool whole = p0 + 4u <= samples, words = whole && b.load_bytes == 4;
  const int n = whole ? 4 : (int) (samples - p0);
  const uint8_t *in = (const uint8_t *) b.in + 3u * p0;
  uint8_t *out = (uint8_t *) b.out + 3u * p0;
  uint32_t w[4] = { 0, 0, 0, 0 }, t[4];
  if (b.mode != AVOL_ZERO) {
    if (words) {
      aconv_load4<AK_3LE> (in, w);
    } else {
      for (int e = 0; e < 4; e++)
        if (e < n)
          w[e] = aconv_load_w<AK_3LE> (in, (size_t) e);
    }
  }
  if (b.mode == AVOL_SCALE) {
    for (int e = 0; e < 4; e++)
      t[e] = (uint32_t) avol_scale24 ((int32_t) (w[e] << 8) >> 8, b.vol) & 0xffffffu;
  } else if (b.mode == AVOL_GAINS || b.mode == AVOL_GAINS_MUTE) {
    uint32_t frame, channel;
    avol_frame_of (p0, (uint32_t) channels, &frame, &channel);
    for (int e = 0; e < 4; e++) {
      double g = 0.0;
      if (e < n) {
        if (b.mode == AVOL_GAINS)
          g = b.gains[frame];
        if (++channel == (uint32_t) channels)
          channel = 0, frame++;
      }
      t[e] = (uint32_t) avol_gain24 ((int32_t) (w[e] << 8) >> 8, g) & 0xffffffu;
    }
  } else {
    for (int e = 0; e < 4; e++)
      t[e] = w[e];
  }
  if (words) {
    aconv_store4<AK_3LE> (out, t);
  } else {
    for (int e = 0; e < 4; e++)
      if (e < n)
        aconv_store_w<AK_3LE> (out, (size_t) e, t[e]);
  }
}

// the workgroups of one buffer: blockIdx.x = block of gridDim.x = blocks walks its pieces, 256 at a time
template <typename T>
GSTAMD_AC uint64_t avol_buffer_pieces (const AVolBuf &b, int channels)
{
  return avol_pieces ((uint64_t) b.frames * (uint64_t) channels, avol_lead (b.out, (int) sizeof (T)), (int) sizeof (T));
}

}  // namespace gstamd
