// audio_convert_device.h - GstAudioConverter's per-sample stages as device code (bodies only; tests/emu runs the same bodies on the host).
//
// Reference (paths under /root/reference/subprojects/gst-plugins-base/gst-libs/gst/audio/):
//   chain_unpack / _convert_in / _mix / _resample / _convert_out / _quantize / _pack      audio-converter.c:708-1090
//   unpack_* / pack_* of the formats                                                      audio-format.c:117-260, gstaudiopack.orc
//   audio_orc_s32_to_double / audio_orc_double_to_s32                                     gstaudiopack.orc:412-426
//   gst_audio_channel_mixer_mix_{int16,int32,float,double}                                audio-channel-mixer.c:961-1015
//   gst_audio_quantize_quantize_int_none_none / _int_dither_none, setup_dither_buf        audio-quantize.c:83-180
//   gst_fast_random_uint32 (32-bit xorshift)                                              audio-quantize.c:92-100
//
// The plan (AConvPlan) is made on the host by the decision code of audio_convert.hip, which restates gst_audio_converter_new.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/gstamd_audio.h"

#ifdef __HIPCC__
#define GSTAMD_AC __host__ __device__ __forceinline__
#else
#define GSTAMD_AC inline
#endif

namespace gstamd {

// the format the samples are in between the stages (audio-converter.c is_intermediate_format)
enum AMid : int { AMID_S16 = 0, AMID_S32 = 1, AMID_F32 = 2, AMID_F64 = 3 };

struct AConvPlan {
  int in_fmt, out_fmt;          // GSTAMD_AFMT_*
  int in_kind, out_kind;        // AKind: the containers, which the kernels are instantiated for
  int in_shift;                 // integer input: 32 - depth
  uint32_t in_sx;               // integer input: 0x80000000 for the unsigned formats
  int out_shift, out_usgn;      // integer output: 32 - depth, unsigned
  int endian_swap;              // the whole conversion is a byte swap of this many bytes per sample (converter_endian); 0: it is not
  int in_ch, out_ch;
  int mid_in;                   // AMid after unpack (+ convert_in): what the mixer and the resampler work on
  int convert_in;               // S32 -> F64 after unpack
  int mix;                      // 0: the mixer is a passthrough
  int convert_out;              // F64 -> S32 after the resampler
  int mid_out;                  // AMid after convert_out: what quantize / pack see
  int quant_shift;              // 0: no quantize stage
  int dither;                   // GSTAMD_AUDIO_DITHER_* of the quantize stage
  int ns;                       // GSTAMD noise shaping of the quantize stage: 0 none, 1 error feedback, 2.. the filters (n_coeffs taps)
  int n_coeffs;
  int32_t coeffs[8];            // floor (c * 1024 + 0.5), audio-quantize.c:344-373
  float m[GSTAMD_AUDIO_MAX_CHANNELS][GSTAMD_AUDIO_MAX_CHANNELS];        // [in][out]
  int mi[GSTAMD_AUDIO_MAX_CHANNELS][GSTAMD_AUDIO_MAX_CHANNELS];         // (gint) (m * 1024)
  int sparse;                   // the mixer's sparse form: only the coefficients of use[] are summed
  uint32_t use[GSTAMD_AUDIO_MAX_CHANNELS];                              // [out]: bit ci = input channel ci takes part
  int q_stride;                 // samples between two frames of a channel as the quantize stage sees them: out_ch, or 1 for a non-interleaved
                                // output, which gst_audio_quantize_samples walks plane after plane as ONE channel
};

// the caller-facing side of a non-interleaved converter: the planes by value in the kernel arguments.  head[y]: how row y of the launch
// (a plane; for the mixing first kernel an output channel) splits its frames - 0 .. 3 single frames up to the dword boundary the
// four-frame lanes start on (AConvSplit), 4: a lane per frame.  realign: the planes a mixing row reads do not reach a dword boundary at
// the same frame; the four-frame lanes start at frame 4, end four frames or more before the last, and shift what they load (aconv_load4_any).
struct AConvPlanes {
  uint8_t *p[GSTAMD_AUDIO_MAX_CHANNELS];
  size_t frames;
  uint8_t head[GSTAMD_AUDIO_MAX_CHANNELS];
  uint8_t realign;
};

// the same for a converter of up to 64 channels (gstamd_audio_converter_new_wide); 592 bytes of kernel arguments
struct AConvPlanesWide {
  uint8_t *p[GSTAMD_AUDIO_MAX_CHANNELS_WIDE];
  size_t frames;
  uint8_t head[GSTAMD_AUDIO_MAX_CHANNELS_WIDE];
  uint8_t realign;              // 0: the wide first kernel stages every plane on its own, nothing has to line up
};

GSTAMD_AC int amid_bytes (int mid) { return mid == AMID_S16 ? 2 : mid == AMID_F64 ? 8 : 4; }

// ---- the raw GstAudioFormats, values 2 .. 31 (audio-format.h:80-130) --------------------------------------------------------------------------------
// Values 4 .. 27 come in groups of four - LE, BE, unsigned LE, unsigned BE - of one container / depth; 28 .. 31 are F32 / F64, LE then BE.
struct AFmtDesc {
  bool known, integer, usgn, be;
  int depth, bytes;
};

GSTAMD_AC AFmtDesc afmt_desc (int fmt)
{
  if (fmt == GSTAMD_AFMT_S8 || fmt == GSTAMD_AFMT_U8)
    return {true, true, fmt == GSTAMD_AFMT_U8, false, 8, 1};
  if (fmt >= GSTAMD_AFMT_S16LE && fmt <= GSTAMD_AFMT_U18BE) {
    const int g = (fmt - GSTAMD_AFMT_S16LE) >> 2;               /* S16, S24_32, S32, S24, S20, S18 */
    const int depth = g == 0 ? 16 : g == 2 ? 32 : g == 4 ? 20 : g == 5 ? 18 : 24;
    const int bytes = g == 0 ? 2 : g <= 2 ? 4 : 3;
    return {true, true, (fmt & 2) != 0, (fmt & 1) != 0, depth, bytes};
  }
  if (fmt >= GSTAMD_AFMT_F32LE && fmt <= GSTAMD_AFMT_F64BE)
    return {true, false, false, (fmt & 1) != 0, fmt < GSTAMD_AFMT_F64LE ? 32 : 64, fmt < GSTAMD_AFMT_F64LE ? 4 : 8};
  return {false, false, false, false, 0, 0};
}

GSTAMD_AC int afmt_bytes (int fmt) { return afmt_desc (fmt).bytes; }

// What a kernel has to know of a format at compile time is its container: bytes per sample and byte order.  Depth and sign are a shift
// and an xor taken from the plan (uniform over a launch), so the kernels are instantiated per AKind and hold no format switch.
enum AKind : int { AK_1 = 0, AK_2LE, AK_2BE, AK_3LE, AK_3BE, AK_4LE, AK_4BE, AK_8LE, AK_8BE };

GSTAMD_AC constexpr int akind_bytes (int k) { return k == AK_1 ? 1 : k <= AK_2BE ? 2 : k <= AK_3BE ? 3 : k <= AK_4BE ? 4 : 8; }
GSTAMD_AC constexpr bool akind_be (int k) { return k == AK_2BE || k == AK_3BE || k == AK_4BE || k == AK_8BE; }
GSTAMD_AC int afmt_kind (int fmt)
{
  const AFmtDesc d = afmt_desc (fmt);
  return d.bytes == 1 ? AK_1 : (d.bytes == 2 ? AK_2LE : d.bytes == 3 ? AK_3LE : d.bytes == 4 ? AK_4LE : AK_8LE) + (d.be ? 1 : 0);
}

// the switch outside the loop: F (K) with the container as a constant
#define GSTAMD_ACONV_FOR_KIND(kind, F) \
  switch (kind) { \
    case gstamd::AK_1: F (gstamd::AK_1); break; \
    case gstamd::AK_2LE: F (gstamd::AK_2LE); break; \
    case gstamd::AK_2BE: F (gstamd::AK_2BE); break; \
    case gstamd::AK_3LE: F (gstamd::AK_3LE); break; \
    case gstamd::AK_3BE: F (gstamd::AK_3BE); break; \
    case gstamd::AK_4LE: F (gstamd::AK_4LE); break; \
    case gstamd::AK_4BE: F (gstamd::AK_4BE); break; \
    case gstamd::AK_8LE: F (gstamd::AK_8LE); break; \
    default: F (gstamd::AK_8BE); break; \
  }

// ORC's C backups flush denormals around float operations (ORC_DENORMAL / ORC_DENORMAL_DOUBLE, orc/orcprogram-c.c): a value whose
// exponent field is zero keeps only its sign
GSTAMD_AC uint32_t orc_denormal_f (uint32_t x) { return (x & 0x7f800000u) == 0 ? (x & 0xff800000u) : x; }
GSTAMD_AC uint64_t orc_denormal_d (uint64_t x) { return (x & 0x7ff0000000000000ull) == 0 ? (x & 0xfff0000000000000ull) : x; }
GSTAMD_AC double bits_d (uint64_t b) { double d; memcpy (&d, &b, 8); return d; }
GSTAMD_AC uint64_t d_bits (double d) { uint64_t b; memcpy (&b, &d, 8); return b; }
GSTAMD_AC float bits_f (uint32_t b) { float f; memcpy (&f, &b, 4); return f; }
GSTAMD_AC uint32_t f_bits (float f) { uint32_t b; memcpy (&b, &f, 4); return b; }

// v_perm_b32: result byte i is the byte the selector's byte i names - 0 .. 3 of lo, 4 .. 7 of hi, 0x0c a zero byte
GSTAMD_AC uint32_t aconv_perm (uint32_t hi, uint32_t lo, uint32_t sel)
{
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_perm (hi, lo, sel);
#else                           /* the plain C twin: the host emulator of tests/emu, and the host pass of hipcc */
  const uint64_t both = ((uint64_t) hi << 32) | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) {
    const uint32_t s = (sel >> (8 * i)) & 0xffu;
    r |= (s < 8 ? (uint32_t) (both >> (8 * s)) & 0xffu : 0u) << (8 * i);
  }
  return r;
#endif
}
GSTAMD_AC uint32_t aconv_bswap32 (uint32_t v) { return aconv_perm (0u, v, 0x00010203u); }
GSTAMD_AC uint64_t aconv_bswap64 (uint64_t v) { return ((uint64_t) aconv_bswap32 ((uint32_t) v) << 32) | aconv_bswap32 ((uint32_t) (v >> 32)); }

// ---- one sample: the container as an unsigned word in the format's byte order, read and written byte-wise (any address) ---------------
template <int K> GSTAMD_AC uint32_t aconv_load_w (const uint8_t *p, size_t i)
{
  constexpr int B = akind_bytes (K);
  const uint8_t *q = p + (size_t) B * i;
  if constexpr (B == 1) {
    return q[0];
  } else if constexpr (B == 2) {
    return akind_be (K) ? ((uint32_t) q[0] << 8) | q[1] : (uint32_t) q[0] | ((uint32_t) q[1] << 8);
  } else if constexpr (B == 3) {
    return akind_be (K) ? ((uint32_t) q[0] << 16) | ((uint32_t) q[1] << 8) | q[2] : (uint32_t) q[0] | ((uint32_t) q[1] << 8) | ((uint32_t) q[2] << 16);
  } else {
    uint32_t v; memcpy (&v, q, 4);
    return akind_be (K) ? aconv_bswap32 (v) : v;
  }
}

template <int K> GSTAMD_AC uint64_t aconv_load_w64 (const uint8_t *p, size_t i)
{
  uint64_t v; memcpy (&v, p + 8 * i, 8);
  return akind_be (K) ? aconv_bswap64 (v) : v;
}

template <int K> GSTAMD_AC void aconv_store_w (uint8_t *p, size_t i, uint32_t t)
{
  constexpr int B = akind_bytes (K);
  uint8_t *q = p + (size_t) B * i;
  if constexpr (B == 1) {
    q[0] = (uint8_t) t;
  } else if constexpr (B == 2) {
    q[akind_be (K) ? 1 : 0] = (uint8_t) t; q[akind_be (K) ? 0 : 1] = (uint8_t) (t >> 8);
  } else if constexpr (B == 3) {
    q[akind_be (K) ? 2 : 0] = (uint8_t) t; q[1] = (uint8_t) (t >> 8); q[akind_be (K) ? 0 : 2] = (uint8_t) (t >> 16);
  } else {
    const uint32_t v = akind_be (K) ? aconv_bswap32 (t) : t;
    memcpy (q, &v, 4);
  }
}

template <int K> GSTAMD_AC void aconv_store_w64 (uint8_t *p, size_t i, uint64_t t)
{
  const uint64_t v = akind_be (K) ? aconv_bswap64 (t) : t;
  memcpy (p + 8 * i, &v, 8);
}

// N dwords at a 4-byte aligned address (consecutive dword accesses of a lane become one global_load / _store_dwordxN)
typedef uint32_t __attribute__ ((may_alias)) aconv_u32;
template <int N> GSTAMD_AC void aconv_load_words (const void *q, uint32_t *d)
{
  const aconv_u32 *s = (const aconv_u32 *) q;
  for (int j = 0; j < N; j++)
    d[j] = s[j];
}

template <int N> GSTAMD_AC void aconv_store_words (void *q, const uint32_t *d)
{
  aconv_u32 *s = (aconv_u32 *) q;
  for (int j = 0; j < N; j++)
    s[j] = d[j];
}

// ---- four consecutive samples on aligned dwords: 4 samples of a B-byte container are B dwords; q is 4-byte aligned ---------------------
// d: the B dwords that hold four samples -> the four containers
template <int K> GSTAMD_AC void aconv_words_to_w4 (const uint32_t *d, uint32_t w[4])
{
  constexpr int B = akind_bytes (K);
  constexpr bool BE = akind_be (K);
  static_assert (B <= 4, "64-bit containers: aconv_load4_64");
  if constexpr (B == 1) {
    for (int j = 0; j < 4; j++)
      w[j] = (d[0] >> (8 * j)) & 0xffu;
  } else if constexpr (B == 2) {
    for (int j = 0; j < 2; j++) {
      w[2 * j] = BE ? aconv_perm (0u, d[j], 0x0c0c0001u) : d[j] & 0xffffu;
      w[2 * j + 1] = BE ? aconv_perm (0u, d[j], 0x0c0c0203u) : d[j] >> 16;
    }
  } else if constexpr (B == 3) {        /* stream bytes 0 .. 11 = d[0] d[1] d[2]; sample j is bytes 3j .. 3j + 2 */
    w[0] = aconv_perm (0u, d[0], BE ? 0x0c000102u : 0x0c020100u);
    w[1] = aconv_perm (d[1], d[0], BE ? 0x0c030405u : 0x0c050403u);
    w[2] = aconv_perm (d[2], d[1], BE ? 0x0c020304u : 0x0c040302u);
    w[3] = aconv_perm (0u, d[2], BE ? 0x0c010203u : 0x0c030201u);
  } else {
    for (int j = 0; j < 4; j++)
      w[j] = BE ? aconv_bswap32 (d[j]) : d[j];
  }
}

template <int K> GSTAMD_AC void aconv_load4 (const uint8_t *q, uint32_t w[4])
{
  constexpr int B = akind_bytes (K);
  uint32_t d[B];
  aconv_load_words<B> (q, d);
  aconv_words_to_w4<K> (d, w);
}

// the same at any address: the B + 1 aligned dwords around the four samples, shifted down by the address' byte phase.  The caller
// keeps [q - 3, q + 4 B + 4) inside the buffer (aconv_plane_split leaves four frames to single lanes at both ends of a plane for that).
template <int K> GSTAMD_AC void aconv_load4_any (const uint8_t *q, uint32_t w[4])
{
  constexpr int B = akind_bytes (K);
  if constexpr (B >= 4) {               /* samples of four bytes are aligned */
    aconv_load4<K> (q, w);
  } else {
    const unsigned a = (unsigned) ((uintptr_t) q & 3u);
    uint32_t x[B + 1], d[B];
    aconv_load_words<B + 1> (q - a, x);
    for (int k = 0; k < B; k++)
      d[k] = (uint32_t) (((((uint64_t) x[k + 1]) << 32) | x[k]) >> (8u * a));
    aconv_words_to_w4<K> (d, w);
  }
}

template <int K> GSTAMD_AC void aconv_store4 (uint8_t *q, const uint32_t t[4])
{
  constexpr int B = akind_bytes (K);
  constexpr bool BE = akind_be (K);
  static_assert (B <= 4, "64-bit containers: aconv_store4_64");
  uint32_t d[B];
  if constexpr (B == 1) {
    d[0] = aconv_perm (t[1], t[0], 0x0c0c0400u) | aconv_perm (t[3], t[2], 0x04000c0cu);
  } else if constexpr (B == 2) {
    d[0] = aconv_perm (t[1], t[0], BE ? 0x04050001u : 0x05040100u);
    d[1] = aconv_perm (t[3], t[2], BE ? 0x04050001u : 0x05040100u);
  } else if constexpr (B == 3) {
    d[0] = aconv_perm (t[1], t[0], BE ? 0x06000102u : 0x04020100u);
    d[1] = aconv_perm (t[2], t[1], BE ? 0x05060001u : 0x05040201u);
    d[2] = aconv_perm (t[3], t[2], BE ? 0x04050600u : 0x06050402u);
  } else {
    for (int j = 0; j < 4; j++)
      d[j] = BE ? aconv_bswap32 (t[j]) : t[j];
  }
  aconv_store_words<B> (q, d);
}

template <int K> GSTAMD_AC void aconv_load4_64 (const uint8_t *q, uint64_t w[4])
{
  uint32_t d[8];
  aconv_load_words<8> (q, d);
  for (int j = 0; j < 4; j++)
    w[j] = akind_be (K) ? ((uint64_t) aconv_bswap32 (d[2 * j]) << 32) | aconv_bswap32 (d[2 * j + 1]) : ((uint64_t) d[2 * j + 1] << 32) | d[2 * j];
}

template <int K> GSTAMD_AC void aconv_store4_64 (uint8_t *q, const uint64_t t[4])
{
  uint32_t d[8];
  for (int j = 0; j < 4; j++) {
    const uint32_t lo = (uint32_t) t[j], hi = (uint32_t) (t[j] >> 32);
    d[2 * j] = akind_be (K) ? aconv_bswap32 (hi) : lo;
    d[2 * j + 1] = akind_be (K) ? aconv_bswap32 (lo) : hi;
  }
  aconv_store_words<8> (q, d);
}

// How the lanes of a launch share n consecutive samples of a caller's buffer: `head` single samples up to the first dword boundary on
// which a sample starts, then `groups` lanes of four samples on aligned dwords, the rest single again.  groups == 0: a lane per sample.
struct AConvSplit {
  size_t head, groups, n;
};

inline AConvSplit aconv_split (const void *buf, int bytes, size_t n, bool grouped)
{
  AConvSplit s = { 0, 0, n };
  size_t h = 0;
  while (h < 4 && (((uintptr_t) buf + (size_t) bytes * h) & 3u))
    h++;
  if (!grouped || h == 4 || n < h + 4)          /* h == 4: no sample of this buffer starts on a dword */
    return s;
  s.head = h;
  s.groups = (n - h) / 4;
  return s;
}

GSTAMD_AC size_t aconv_split_lanes (const AConvSplit &s) { return s.groups + (s.n - 4 * s.groups); }
// lane t >= groups: the single sample it takes
GSTAMD_AC size_t aconv_split_single (const AConvSplit &s, size_t t)
{
  const size_t k = t - s.groups;
  return k < s.head ? k : k + 4 * s.groups;
}

// head of aconv_split's grouped form for n samples at q, or 4 where no lane of four samples fits: the same decision on the device
GSTAMD_AC int aconv_head_at (const uint8_t *q, int bytes, size_t n)
{
  int h = 0;
  while (h < 4 && (((uintptr_t) q + (size_t) (bytes * h)) & 3u))
    h++;
  return h == 4 || n < (size_t) h + 4 ? 4 : h;
}

// A non-interleaved side as gstamd_audio_converter_samples takes it: ONE pointer, the planes frames * bytes apart.  No pointer array,
// so it is made in registers from a 16-byte table entry (AConvManySide) and serves any channel count.  how: 0 .. 4 is the
// head of every row (a mixing first kernel: aconv_planes_heads' "same" rule, decided on the host); AConvPlanesEven::OWN: row y works on
// plane y alone and takes the head of that plane's address.
struct AConvPlanesEven {
  enum { OWN = 5 };
  uint8_t *base;
  size_t frames;
  int bytes;                    // of a sample
  int how;
  int realign;                  // as in AConvPlanes
};

// what the lane bodies ask of a planes struct beside .frames and .realign
GSTAMD_AC uint8_t *aconv_plane_ptr (const AConvPlanes &pl, int c) { return pl.p[c]; }
GSTAMD_AC uint8_t *aconv_plane_ptr (const AConvPlanesWide &pl, int c) { return pl.p[c]; }
GSTAMD_AC uint8_t *aconv_plane_ptr (const AConvPlanesEven &pl, int c) { return pl.base + (size_t) c * pl.frames * (size_t) pl.bytes; }
GSTAMD_AC int aconv_plane_head (const AConvPlanes &pl, int y) { return pl.head[y]; }
GSTAMD_AC int aconv_plane_head (const AConvPlanesWide &pl, int y) { return pl.head[y]; }
GSTAMD_AC int aconv_plane_head (const AConvPlanesEven &pl, int y)
{
  return pl.how == AConvPlanesEven::OWN ? aconv_head_at (aconv_plane_ptr (pl, y), pl.bytes, pl.frames) : pl.how;
}

// ---- unpack / pack (audio-format.c unpack_* / pack_*, gstaudiopack.orc) ------------------------------------------------------------------
// do_unpack passes GST_AUDIO_PACK_FLAG_TRUNCATE_RANGE (audio-converter.c:477): the *_trunc programs, plain shifts.  Integer container w
// of depth d -> S32: w << (32 - d), sign bit flipped for the unsigned formats; container bits above the depth fall off the top.
GSTAMD_AC int32_t aconv_w_to_s32 (const AConvPlan &p, uint32_t w) { return (int32_t) ((w << p.in_shift) ^ p.in_sx); }

// S32 -> container: signed formats shift arithmetically (the spare bits of S24_32 / S20 / S18 carry the sign), unsigned ones flip the
// sign bit and shift logically (spare bits zero)
GSTAMD_AC uint32_t aconv_s32_to_w (const AConvPlan &p, int32_t v)
{
  return p.out_usgn ? ((uint32_t) v ^ 0x80000000u) >> p.out_shift : (uint32_t) (v >> p.out_shift);
}

// audio_orc_unpack_f32: convfd with the denormal flush; f64: a copy
GSTAMD_AC double aconv_f32w_to_double (uint32_t b) { return (double) bits_f (orc_denormal_f (b)); }

// audio_orc_pack_f32: convdf, denormals flushed on both sides
GSTAMD_AC uint32_t aconv_double_to_f32w (double v)
{
  const float f = (float) bits_d (orc_denormal_d (d_bits (v)));
  return orc_denormal_f (f_bits (f));
}

// sample i of a buffer of container K, unpacked to S32 (integer formats)
template <int K> GSTAMD_AC int32_t aconv_unpack_int (const AConvPlan &p, const uint8_t *in, size_t i)
{
  if constexpr (akind_bytes (K) <= 4)
    return aconv_w_to_s32 (p, aconv_load_w<K> (in, i));
  else
    return 0;
}

// sample i of a float buffer, unpacked to F64
template <int K> GSTAMD_AC double aconv_unpack_flt (const uint8_t *in, size_t i)
{
  if constexpr (akind_bytes (K) == 4)
    return aconv_f32w_to_double (aconv_load_w<K> (in, i));
  else if constexpr (akind_bytes (K) == 8)
    return bits_d (aconv_load_w64<K> (in, i));
  else
    return 0.0;
}

template <int K> GSTAMD_AC void aconv_pack_int (const AConvPlan &p, uint8_t *out, size_t i, int32_t v)
{
  if constexpr (akind_bytes (K) <= 4)
    aconv_store_w<K> (out, i, aconv_s32_to_w (p, v));
}

template <int K> GSTAMD_AC void aconv_pack_flt (uint8_t *out, size_t i, double v)
{
  if constexpr (akind_bytes (K) == 4)
    aconv_store_w<K> (out, i, aconv_double_to_f32w (v));
  else if constexpr (akind_bytes (K) == 8)
    aconv_store_w64<K> (out, i, d_bits (v));
}

// audio_orc_s32_to_double: convld, divd 2147483648.0
GSTAMD_AC double aconv_s32_to_double (int32_t s)
{
  return bits_d (orc_denormal_d (d_bits ((double) s / 2147483648.0)));
}

// audio_orc_double_to_s32: muld 2147483648.0, convdl (the C backup: (int) x, and 0x80000000 from a non-negative x becomes 0x7fffffff)
GSTAMD_AC int32_t aconv_double_to_s32 (double x)
{
  const double a = bits_d (orc_denormal_d (d_bits (x)));
  const double t = bits_d (orc_denormal_d (d_bits (a * 2147483648.0)));
  if (!(t == t))                                /* NaN: the conversion gives 0x80000000, the fix-up looks at the sign bit */
    return (d_bits (t) >> 63) ? (int32_t) 0x80000000u : 0x7fffffff;
  if (t >= 2147483648.0)
    return 0x7fffffff;
  if (t <= -2147483649.0)
    return (int32_t) 0x80000000u;
  return (int32_t) t;
}

GSTAMD_AC int32_t aconv_addssl (int32_t a, int32_t b)
{
  const int64_t s = (int64_t) a + (int64_t) b;
  return s > 2147483647ll ? 2147483647 : (s < -2147483648ll ? (int32_t) 0x80000000u : (int32_t) s);
}

// ---- the 32-bit xorshift of audio-quantize.c and jumping ahead in it -----------------------------------------------------------------
GSTAMD_AC uint32_t aconv_rand_step (uint32_t s)
{
  uint64_t x = s;
  x ^= x << 13;
  x ^= x >> 17;
  x ^= x << 5;
  return (uint32_t) x;
}

// The step is linear over GF(2); jump[j] holds the images of the 32 unit vectors under 2^j steps, so k steps are at most 32
// matrix-vector products.  (Filled on the host by aconv_make_jump.)
struct AConvJump {
  uint32_t col[32][32];
};

GSTAMD_AC uint32_t aconv_rand_jump (const AConvJump &j, uint32_t s, uint64_t k)
{
  for (int b = 0; b < 32 && (k >> b); b++) {
    if (!((k >> b) & 1))
      continue;
    uint32_t r = 0;
    for (int i = 0; i < 32; i++)
      if ((s >> i) & 1)
        r ^= j.col[b][i];
    s = r;
  }
  return s;
}

inline void aconv_make_jump (AConvJump *j)
{
  for (int i = 0; i < 32; i++)
    j->col[0][i] = aconv_rand_step (1u << i);
  for (int b = 1; b < 32; b++)
    for (int i = 0; i < 32; i++) {
      uint32_t s = j->col[b - 1][i], r = 0;     /* apply the 2^(b-1) map twice */
      for (int q = 0; q < 32; q++)
        if ((s >> q) & 1)
          r ^= j->col[b - 1][q];
      j->col[b][i] = r;
    }
}

// RANDOM_INT_DITHER (state, dither): -dither + (next () & (2 dither - 1))
GSTAMD_AC int32_t aconv_random_dither (uint32_t *state, int32_t dither)
{
  *state = aconv_rand_step (*state);
  return -dither + (int32_t) (*state & (uint32_t) ((dither << 1) - 1));
}

// the generator across calls: its state before this call's draws, and - for tpdf-hf, whose value at a sample is the difference to the
// draw of the previous frame's sample of the same channel (last_random) - the state before the draws of the previous call's last frame
struct AConvDitherState {
  uint32_t state0;
  uint32_t prev_state;
  int has_prev;                 // 0: last_random is still the zeros of gst_audio_quantize_setup_dither
};

// setup_dither_buf (audio-quantize.c:117-170): the dither word of sample index i of the call (the order the quantizer walks the call's samples
// in - interleaved, or plane after plane -, draws in that order)
GSTAMD_AC int32_t aconv_dither_value (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, size_t i)
{
  const int shift = p.quant_shift;
  const uint32_t bias = 1u << (shift - 1);
  switch (p.dither) {
    case GSTAMD_AUDIO_DITHER_RPDF: {
      uint32_t st = aconv_rand_jump (jump, ds.state0, (uint64_t) i);
      return (int32_t) (bias + (uint32_t) aconv_random_dither (&st, 1 << shift));
    }
    case GSTAMD_AUDIO_DITHER_TPDF: {
      uint32_t st = aconv_rand_jump (jump, ds.state0, 2 * (uint64_t) i);
      const int32_t r1 = aconv_random_dither (&st, 1 << (shift - 1));
      const int32_t r2 = aconv_random_dither (&st, 1 << (shift - 1));
      return (int32_t) (bias + (uint32_t) r1 + (uint32_t) r2);
    }
    case GSTAMD_AUDIO_DITHER_TPDF_HF: {
      const size_t stride = (size_t) p.q_stride;
      uint32_t st = aconv_rand_jump (jump, ds.state0, (uint64_t) i);
      const int32_t tmp = aconv_random_dither (&st, 1 << (shift - 1));
      int32_t last = 0;
      if (i >= stride) {
        uint32_t s2 = aconv_rand_jump (jump, ds.state0, (uint64_t) (i - stride));
        last = aconv_random_dither (&s2, 1 << (shift - 1));
      } else if (ds.has_prev) {
        uint32_t s2 = aconv_rand_jump (jump, ds.prev_state, (uint64_t) i);
        last = aconv_random_dither (&s2, 1 << (shift - 1));
      }
      return (int32_t) (bias + (uint32_t) tmp - (uint32_t) last);
    }
    default:
      /* no dither: audio_orc_int_bias adds the bias; with noise shaping the quantizer reads a dither buffer of zeros instead */
      return p.ns ? 0 : (int32_t) bias;
  }
}

// draws of a call over `samples` samples
GSTAMD_AC uint64_t aconv_dither_draws (const AConvPlan &p, size_t samples)
{
  if (p.quant_shift <= 0 || p.dither == GSTAMD_AUDIO_DITHER_NONE)
    return 0;
  return (uint64_t) samples * (p.dither == GSTAMD_AUDIO_DITHER_TPDF ? 2u : 1u);
}

// after a call: the generator has moved on by the call's draws (host side)
inline void aconv_dither_advance (const AConvPlan &p, const AConvJump &jump, AConvDitherState *ds, size_t samples)
{
  if (samples == 0 || aconv_dither_draws (p, samples) == 0)
    return;
  if (p.dither == GSTAMD_AUDIO_DITHER_TPDF_HF) {
    ds->prev_state = aconv_rand_jump (jump, ds->state0, (uint64_t) (samples - (size_t) p.q_stride));
    ds->has_prev = 1;
  }
  ds->state0 = aconv_rand_jump (jump, ds->state0, aconv_dither_draws (p, samples));
}

// quantize stage without noise shaping: gst_audio_quantize_quantize_int_none_none / _int_dither_none
GSTAMD_AC int32_t aconv_quantize (const AConvPlan &p, int32_t d, int32_t v)
{
  const uint32_t mask = ~((1u << p.quant_shift) - 1u);
  return (int32_t) ((uint32_t) aconv_addssl (v, d) & mask);
}

// quantize stage with noise shaping for channel c of a call: the error recurrence runs down the frames (one lane per channel).
// v / d: the call's S32 samples and dither words; hist: [8][channels] error history carried between calls (zeros after new / reset).
//   gst_audio_quantize_quantize_int_dither_feedback      audio-quantize.c:199-231
//   gst_audio_quantize_quantize_int_dither_noise_shape   audio-quantize.c:239-278
template <int K> GSTAMD_AC void aconv_shape_channel (const AConvPlan &p, const int32_t *v, const int32_t *d, int32_t *hist, uint8_t *out, size_t frames, int c)
{
  const size_t ch = (size_t) p.q_stride;
  const uint32_t mask = ~((1u << p.quant_shift) - 1u);
  if (p.ns == 1) {
    uint32_t e = (uint32_t) hist[c];
    for (size_t n = 0; n < frames; n++) {
      const size_t i = n * ch + (size_t) c;
      const int32_t o = v[i];
      const int32_t err = (int32_t) ((uint32_t) d[i] - e);
      const int32_t x = (int32_t) ((uint32_t) aconv_addssl (o, err) & mask);
      e += (uint32_t) x - (uint32_t) o;
      aconv_pack_int<K> (p, out, i, x);
    }
    hist[c] = (int32_t) e;
    return;
  }
  uint32_t h[8];
  for (int j = 0; j < 8; j++)
    h[j] = j < p.n_coeffs ? (uint32_t) hist[(size_t) j * ch + (size_t) c] : 0u;
  for (size_t n = 0; n < frames; n++) {
    const size_t i = n * ch + (size_t) c;
    uint32_t acc = 0;
    for (int j = 0; j < 8; j++)
      if (j < p.n_coeffs)
        acc -= h[j] * (uint32_t) p.coeffs[j];
    const int32_t err = (int32_t) (acc + 2u) >> 2;              /* (err + SROUND) >> SREDUCE */
    const int32_t o = aconv_addssl (v[i], err);
    const int32_t x = (int32_t) ((uint32_t) aconv_addssl (o, d[i]) & mask);
    const int32_t ne = (int32_t) ((uint32_t) x - (uint32_t) o + 128u) >> 8;      /* (v - o + RROUND) >> REDUCE */
    for (int j = 0; j < 7; j++)
      if (j + 1 < p.n_coeffs)
        h[j] = h[j + 1];
    h[p.n_coeffs - 1] = (uint32_t) ne;
    aconv_pack_int<K> (p, out, i, x);
  }
  for (int j = 0; j < p.n_coeffs; j++)
    hist[(size_t) j * ch + (size_t) c] = (int32_t) h[j];
}

// ---- where sample (frame n, channel ci) of the caller's input is: interleaved frames, or one plane per channel -------------------------
struct AConvSrcFrames {
  const uint8_t *in;
  GSTAMD_AC const uint8_t *at (const AConvPlan &p, int bytes, size_t n, int ci) const { return in + (size_t) bytes * (n * (size_t) p.in_ch + (size_t) ci); }
};

template <class PL> struct AConvSrcPlanesOf {
  const PL &pl;
  GSTAMD_AC const uint8_t *at (const AConvPlan &, int bytes, size_t n, int ci) const { return aconv_plane_ptr (pl, ci) + (size_t) bytes * n; }
};
typedef AConvSrcPlanesOf<AConvPlanes> AConvSrcPlanes;

// ---- stage 1: input frame n, output channel co -> one sample in the mid_in format (the mid buffers are interleaved frames) --------------
template <int K, class Src> GSTAMD_AC void aconv_pre_sample_at (const AConvPlan &p, const Src &src, uint8_t *mid, size_t n, int co)
{
  constexpr int B = akind_bytes (K);
  const size_t o = n * (size_t) p.out_ch + (size_t) co;
  switch (p.mid_in) {
    case AMID_S16: {            // same 16-bit format in and out: the samples themselves
      int32_t res;
      if (!p.mix) {
        int16_t v; memcpy (&v, src.at (p, 2, n, co), 2);
        res = v;
      } else {
        res = 0;
        for (int ci = 0; ci < p.in_ch; ci++) {
          if (!((p.use[co] >> ci) & 1u))
            continue;
          int16_t v; memcpy (&v, src.at (p, 2, n, ci), 2);
          res += (int32_t) v * p.mi[ci][co];
        }
        res = (res + 512) >> 10;
        res = res > 32767 ? 32767 : (res < -32768 ? -32768 : res);
      }
      const int16_t r = (int16_t) res;
      memcpy (mid + 2 * o, &r, 2);
      break;
    }
    case AMID_S32: {
      int32_t r;
      if (!p.mix) {
        r = aconv_unpack_int<K> (p, src.at (p, B, n, co), 0);
      } else {
        int64_t res = 0;
        for (int ci = 0; ci < p.in_ch; ci++)
          if ((p.use[co] >> ci) & 1u)
            res += (int64_t) aconv_unpack_int<K> (p, src.at (p, B, n, ci), 0) * (int64_t) p.mi[ci][co];
        res = (res + 512) >> 10;
        r = res > 2147483647ll ? 2147483647 : (res < -2147483648ll ? (int32_t) 0x80000000u : (int32_t) res);
      }
      memcpy (mid + 4 * o, &r, 4);
      break;
    }
    case AMID_F32: {            // F32 in and out: the mixer works in single precision
      float r;
      if (!p.mix) {
        memcpy (&r, src.at (p, 4, n, co), 4);
      } else {
        r = 0.0f;
        for (int ci = 0; ci < p.in_ch; ci++) {
          if (!((p.use[co] >> ci) & 1u))
            continue;
          float v; memcpy (&v, src.at (p, 4, n, ci), 4);
          r += v * p.m[ci][co];
        }
      }
      memcpy (mid + 4 * o, &r, 4);
      break;
    }
    default: {
      double r;
      if (!p.mix) {
        r = p.convert_in ? aconv_s32_to_double (aconv_unpack_int<K> (p, src.at (p, B, n, co), 0)) : aconv_unpack_flt<K> (src.at (p, B, n, co), 0);
      } else {
        r = 0.0;
        for (int ci = 0; ci < p.in_ch; ci++) {
          if (!((p.use[co] >> ci) & 1u))
            continue;
          const double v = p.convert_in ? aconv_s32_to_double (aconv_unpack_int<K> (p, src.at (p, B, n, ci), 0)) : aconv_unpack_flt<K> (src.at (p, B, n, ci), 0);
          r += v * p.m[ci][co];
        }
      }
      memcpy (mid + 8 * o, &r, 8);
      break;
    }
  }
}

template <int K> GSTAMD_AC void aconv_pre_sample (const AConvPlan &p, const uint8_t *in, uint8_t *mid, size_t n, int co)
{
  aconv_pre_sample_at<K> (p, AConvSrcFrames { in }, mid, n, co);
}

// four consecutive samples of the caller's buffer (q on a dword; ANY: wherever they are, aconv_load4_any) in the mid_in format: S32 ...
template <int K, bool ANY = false> GSTAMD_AC void aconv_unpack4_s32 (const AConvPlan &p, const uint8_t *q, int32_t r[4])
{
  if constexpr (akind_bytes (K) <= 4) {
    uint32_t w[4];
    if constexpr (ANY)
      aconv_load4_any<K> (q, w);
    else
      aconv_load4<K> (q, w);
    for (int j = 0; j < 4; j++)
      r[j] = aconv_w_to_s32 (p, w[j]);
  } else {                              /* the 64-bit containers are float formats: the plan never puts S32 behind them */
    for (int j = 0; j < 4; j++)
      r[j] = 0;
  }
}

// ... or F64 (convert_in after an integer unpack, or the float unpack)
template <int K, bool ANY = false> GSTAMD_AC void aconv_unpack4_f64 (const AConvPlan &p, const uint8_t *q, double r[4])
{
  if constexpr (akind_bytes (K) <= 4) {
    uint32_t w[4];
    if constexpr (ANY)
      aconv_load4_any<K> (q, w);
    else
      aconv_load4<K> (q, w);
    for (int j = 0; j < 4; j++)
      r[j] = p.convert_in ? aconv_s32_to_double (aconv_w_to_s32 (p, w[j])) : aconv_f32w_to_double (w[j]);
  } else {
    uint64_t w[4];
    aconv_load4_64<K> (q, w);
    for (int j = 0; j < 4; j++)
      r[j] = bits_d (w[j]);
  }
}

// a lane of the first kernel.  Without a mix, output sample i is input sample i, and a lane of the grouped part takes four of them:
// B dwords of the caller's buffer in, 4 (S32) or 8 (F64) dwords of the mid buffer out.
template <int K> GSTAMD_AC void aconv_pre_lane (const AConvPlan &p, const uint8_t *in, uint8_t *mid, const AConvSplit &s, size_t t)
{
  if (t >= s.groups) {
    const size_t i = aconv_split_single (s, t);
    aconv_pre_sample<K> (p, in, mid, i / (size_t) p.out_ch, (int) (i % (size_t) p.out_ch));
    return;
  }
  constexpr int B = akind_bytes (K);
  const size_t i = s.head + 4 * t;
  const uint8_t *q = in + (size_t) B * i;
  if (p.mid_in == AMID_S32) {
    int32_t r[4];
    uint32_t rw[4];
    aconv_unpack4_s32<K> (p, q, r);
    for (int j = 0; j < 4; j++)
      rw[j] = (uint32_t) r[j];
    aconv_store_words<4> (mid + 4 * i, rw);
    return;
  }
  double r[4];
  aconv_unpack4_f64<K> (p, q, r);
  uint32_t rw[8];
  memcpy (rw, r, 32);
  aconv_store_words<8> (mid + 8 * i, rw);
}

// the mixer's saturating ends (gst_audio_channel_mixer_mix_int32)
GSTAMD_AC int32_t aconv_mix_round_s32 (int64_t res)
{
  res = (res + 512) >> 10;
  return res > 2147483647ll ? 2147483647 : (res < -2147483648ll ? (int32_t) 0x80000000u : (int32_t) res);
}

// the mixing first kernel on interleaved frames: lane t of output channel co takes four whole frames - in_ch runs of four samples, B
// aligned dwords each - and adds every sample to the sum of its frame; a frame's samples come by in ascending channel order, so the sums
// are those of aconv_pre_sample_at.  s: the split of the FRAMES (aconv_split with in_ch * B bytes a frame).
template <int K> GSTAMD_AC void aconv_pre_lane_mix (const AConvPlan &p, const uint8_t *in, uint8_t *mid, const AConvSplit &s, int co, size_t t)
{
  if (t >= aconv_split_lanes (s))
    return;
  if (t >= s.groups) {
    aconv_pre_sample<K> (p, in, mid, aconv_split_single (s, t), co);
    return;
  }
  constexpr int B = akind_bytes (K);
  const size_t n = s.head + 4 * t, och = (size_t) p.out_ch;
  const uint8_t *q = in + (size_t) B * n * (size_t) p.in_ch;
  const uint32_t use = p.use[co];
  int f = 0, ci = 0;                    /* frame (of the lane's four) and channel of the next sample */
  if (p.mid_in == AMID_S32) {
    int64_t res[4] = { 0, 0, 0, 0 };
    for (int g = 0; g < p.in_ch; g++) {
      int32_t r[4];
      aconv_unpack4_s32<K> (p, q + (size_t) (4 * B) * (size_t) g, r);
      for (int jj = 0; jj < 4; jj++) {
        if ((use >> ci) & 1u) {
          const int64_t x = (int64_t) r[jj] * (int64_t) p.mi[ci][co];
          for (int j = 0; j < 4; j++)
            res[j] = f == j ? res[j] + x : res[j];
        }
        if (++ci == p.in_ch) {
          ci = 0;
          f++;
        }
      }
    }
    for (int j = 0; j < 4; j++) {
      const int32_t r = aconv_mix_round_s32 (res[j]);
      memcpy (mid + 4 * ((n + (size_t) j) * och + (size_t) co), &r, 4);
    }
    return;
  }
  double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
  for (int g = 0; g < p.in_ch; g++) {
    double r[4];
    aconv_unpack4_f64<K> (p, q + (size_t) (4 * B) * (size_t) g, r);
    for (int jj = 0; jj < 4; jj++) {
      if ((use >> ci) & 1u) {
        const double x = r[jj] * p.m[ci][co];
        for (int j = 0; j < 4; j++)
          acc[j] = f == j ? acc[j] + x : acc[j];
      }
      if (++ci == p.in_ch) {
        ci = 0;
        f++;
      }
    }
  }
  for (int j = 0; j < 4; j++)
    memcpy (mid + 8 * ((n + (size_t) j) * och + (size_t) co), &acc[j], 8);
}

// the first kernel's lanes can take four samples each: no mix (so no gather over the input channels), S32 or F64 behind it
GSTAMD_AC bool aconv_pre_grouped (const AConvPlan &p) { return !p.mix && (p.mid_in == AMID_S32 || p.mid_in == AMID_F64); }
GSTAMD_AC bool aconv_post_grouped (const AConvPlan &p) { return p.mid_in == AMID_S32 || p.mid_in == AMID_F64; }

// ---- stage 2: sample i (interleaved index) of the mid buffer after the resampler -> the output format -----------------------------
// convert_out and the quantize stage without noise shaping: the S32 sample that is packed.  With noise shaping (returns true) the
// sample and its dither word are for aconv_shape_channel instead.  i: the sample's place in the mid buffer; qi: its place in the order
// the quantizer walks the call in (the same for an interleaved output; plane * frames + frame for a non-interleaved one).
GSTAMD_AC bool aconv_post_int (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, const uint8_t *mid, size_t i, size_t qi, int32_t *v, int32_t *d)
{
  if (p.convert_out) {
    double x; memcpy (&x, mid + 8 * i, 8);
    *v = aconv_double_to_s32 (x);
  } else {
    memcpy (v, mid + 4 * i, 4);
  }
  if (p.quant_shift > 0) {
    *d = aconv_dither_value (p, jump, ds, qi);
    if (p.ns)
      return true;
    *v = aconv_quantize (p, *d, *v);
  }
  return false;
}

// dst: where the packed sample goes
template <int K> GSTAMD_AC void aconv_post_sample_at (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, const uint8_t *mid, size_t i, uint8_t *dst,
    int32_t *qv, int32_t *qd, size_t qi)
{
  if (p.mid_in == AMID_S16) {
    memcpy (dst, mid + 2 * i, 2);
    return;
  }
  if (p.mid_in == AMID_F32) {
    memcpy (dst, mid + 4 * i, 4);
    return;
  }
  if (p.mid_out == AMID_F64) {
    double v; memcpy (&v, mid + 8 * i, 8);
    aconv_pack_flt<K> (dst, 0, v);
    return;
  }
  int32_t v, d = 0;
  if (aconv_post_int (p, jump, ds, mid, i, qi, &v, &d)) {
    qv[qi] = v;
    qd[qi] = d;
    return;
  }
  aconv_pack_int<K> (p, dst, 0, v);
}

template <int K> GSTAMD_AC void aconv_post_sample (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, const uint8_t *mid, uint8_t *out, int32_t *qv,
    int32_t *qd, size_t i)
{
  aconv_post_sample_at<K> (p, jump, ds, mid, i, out + (size_t) akind_bytes (K) * i, qv, qd, i);
}

// a lane of the second kernel; a lane of the grouped part writes four samples as B dwords of the caller's buffer
template <int K> GSTAMD_AC void aconv_post_lane (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, const uint8_t *mid, uint8_t *out, int32_t *qv,
    int32_t *qd, const AConvSplit &s, size_t t)
{
  if (t >= s.groups) {
    aconv_post_sample<K> (p, jump, ds, mid, out, qv, qd, aconv_split_single (s, t));
    return;
  }
  constexpr int B = akind_bytes (K);
  const size_t i = s.head + 4 * t;
  uint8_t *q = out + (size_t) B * i;
  if (p.mid_out == AMID_F64) {
    double v[4];
    uint32_t vw[8];
    aconv_load_words<8> (mid + 8 * i, vw);
    memcpy (v, vw, 32);
    if constexpr (B == 4) {
      uint32_t w[4];
      for (int j = 0; j < 4; j++)
        w[j] = aconv_double_to_f32w (v[j]);
      aconv_store4<K> (q, w);
    } else if constexpr (B == 8) {
      uint64_t w[4];
      for (int j = 0; j < 4; j++)
        w[j] = d_bits (v[j]);
      aconv_store4_64<K> (q, w);
    }
    return;
  }
  if constexpr (B <= 4) {
    int32_t v[4], d[4] = { 0, 0, 0, 0 };
    bool shaped = false;
    for (int j = 0; j < 4; j++)
      shaped = aconv_post_int (p, jump, ds, mid, i + (size_t) j, i + (size_t) j, &v[j], &d[j]);       /* (uniform over the launch) */
    if (shaped) {
      for (int j = 0; j < 4; j++) {
        qv[i + (size_t) j] = v[j];
        qd[i + (size_t) j] = d[j];
      }
      return;
    }
    uint32_t w[4];
    for (int j = 0; j < 4; j++)
      w[j] = aconv_s32_to_w (p, v[j]);
    aconv_store4<K> (q, w);
  }
}

// ---- a non-interleaved side: row y of a launch is a plane, its lanes take four consecutive frames of it on aligned dwords (the unpack /
// pack bodies above as they are) or one frame; what is strided is the interleaved mid buffer ---------------------------------------
template <class PL> GSTAMD_AC AConvSplit aconv_plane_split_of (const PL &pl, int y)
{
  AConvSplit s = { 0, 0, pl.frames };
  if (pl.realign) {                     /* (frames >= 12: aconv_planes_heads) */
    s.head = 4;
    s.groups = (pl.frames - 8) / 4;
  } else {
    const int head = aconv_plane_head (pl, y);
    if (head < 4 && pl.frames >= (size_t) head + 4) {
      s.head = (size_t) head;
      s.groups = (pl.frames - s.head) / 4;
    }
  }
  return s;
}

GSTAMD_AC AConvSplit aconv_plane_split (const AConvPlanes &pl, int y) { return aconv_plane_split_of (pl, y); }

// the first kernel: lane t of output channel co.  The mixer's sums run over the input planes in ascending order as in aconv_pre_sample_at;
// a four-frame lane reads B dwords of every plane it uses - aligned ones where all planes reach a dword boundary at the same frame
// (aconv_planes_heads), B + 1 around its frames otherwise (ANY)
template <int K, bool ANY, class PL> GSTAMD_AC void aconv_pre_group_planes (const AConvPlan &p, const PL &src, uint8_t *mid, int co, size_t n)
{
  constexpr int B = akind_bytes (K);
  const size_t och = (size_t) p.out_ch;
  const uint32_t use = p.mix ? p.use[co] : 1u << co;
  if (p.mid_in == AMID_S32) {
    int64_t res[4] = { 0, 0, 0, 0 };
    int32_t r[4] = { 0, 0, 0, 0 };
    for (int ci = 0; ci < p.in_ch; ci++) {
      if (!((use >> ci) & 1u))
        continue;
      aconv_unpack4_s32<K, ANY> (p, aconv_plane_ptr (src, ci) + (size_t) B * n, r);
      for (int j = 0; j < 4; j++)
        res[j] += (int64_t) r[j] * (int64_t) p.mi[ci][co];
    }
    for (int j = 0; j < 4; j++) {
      const int32_t x = p.mix ? aconv_mix_round_s32 (res[j]) : r[j];
      memcpy (mid + 4 * ((n + (size_t) j) * och + (size_t) co), &x, 4);
    }
    return;
  }
  double acc[4] = { 0.0, 0.0, 0.0, 0.0 }, r[4] = { 0.0, 0.0, 0.0, 0.0 };
  for (int ci = 0; ci < p.in_ch; ci++) {
    if (!((use >> ci) & 1u))
      continue;
    aconv_unpack4_f64<K, ANY> (p, aconv_plane_ptr (src, ci) + (size_t) B * n, r);
    for (int j = 0; j < 4; j++)
      acc[j] += r[j] * p.m[ci][co];
  }
  for (int j = 0; j < 4; j++) {
    const double x = p.mix ? acc[j] : r[j];
    memcpy (mid + 8 * ((n + (size_t) j) * och + (size_t) co), &x, 8);
  }
}

template <int K, class PL> GSTAMD_AC void aconv_pre_lane_planes_of (const AConvPlan &p, const PL &src, uint8_t *mid, int co, size_t t)
{
  const AConvSplit s = aconv_plane_split_of (src, co);
  if (t >= aconv_split_lanes (s))
    return;
  if (t >= s.groups) {
    aconv_pre_sample_at<K> (p, AConvSrcPlanesOf<PL> { src }, mid, aconv_split_single (s, t), co);
    return;
  }
  if (src.realign)
    aconv_pre_group_planes<K, true> (p, src, mid, co, s.head + 4 * t);
  else
    aconv_pre_group_planes<K, false> (p, src, mid, co, s.head + 4 * t);
}

template <int K> GSTAMD_AC void aconv_pre_lane_planes (const AConvPlan &p, const AConvPlanes &src, uint8_t *mid, int co, size_t t)
{
  aconv_pre_lane_planes_of<K> (p, src, mid, co, t);
}

// the second kernel: lane t of output plane c (PL: AConvPlanes or AConvPlanesWide)
template <int K, class PL> GSTAMD_AC void aconv_post_lane_planes_of (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, const uint8_t *mid,
    const PL &dst, int32_t *qv, int32_t *qd, int c, size_t t)
{
  const AConvSplit s = aconv_plane_split_of (dst, c);
  if (t >= aconv_split_lanes (s))
    return;
  constexpr int B = akind_bytes (K);
  const size_t och = (size_t) p.out_ch, q0 = (size_t) c * dst.frames;
  if (t >= s.groups) {
    const size_t n = aconv_split_single (s, t);
    aconv_post_sample_at<K> (p, jump, ds, mid, n * och + (size_t) c, aconv_plane_ptr (dst, c) + (size_t) B * n, qv, qd, q0 + n);
    return;
  }
  const size_t n = s.head + 4 * t;
  uint8_t *q = aconv_plane_ptr (dst, c) + (size_t) B * n;
  if (p.mid_out == AMID_F64) {
    double v[4];
    for (int j = 0; j < 4; j++)
      memcpy (&v[j], mid + 8 * ((n + (size_t) j) * och + (size_t) c), 8);
    if constexpr (B == 4) {
      uint32_t w[4];
      for (int j = 0; j < 4; j++)
        w[j] = aconv_double_to_f32w (v[j]);
      aconv_store4<K> (q, w);
    } else if constexpr (B == 8) {
      uint64_t w[4];
      for (int j = 0; j < 4; j++)
        w[j] = d_bits (v[j]);
      aconv_store4_64<K> (q, w);
    }
    return;
  }
  if constexpr (B <= 4) {
    int32_t v[4], d[4] = { 0, 0, 0, 0 };
    bool shaped = false;
    for (int j = 0; j < 4; j++)
      shaped = aconv_post_int (p, jump, ds, mid, (n + (size_t) j) * och + (size_t) c, q0 + n + (size_t) j, &v[j], &d[j]);
    if (shaped) {
      for (int j = 0; j < 4; j++) {
        qv[q0 + n + (size_t) j] = v[j];
        qd[q0 + n + (size_t) j] = d[j];
      }
      return;
    }
    uint32_t w[4];
    for (int j = 0; j < 4; j++)
      w[j] = aconv_s32_to_w (p, v[j]);
    aconv_store4<K> (q, w);
  }
}

template <int K> GSTAMD_AC void aconv_post_lane_planes (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, const uint8_t *mid, const AConvPlanes &dst,
    int32_t *qv, int32_t *qd, int c, size_t t)
{
  aconv_post_lane_planes_of<K> (p, jump, ds, mid, dst, qv, qd, c, t);
}

// noise shaping into a non-interleaved output: ONE recurrence over plane 0, plane 1, ... of the call (the plan's q_stride is 1, the
// history one channel's, carried from each plane into the next)
template <int K, class PL> GSTAMD_AC void aconv_shape_planes_of (const AConvPlan &p, const int32_t *v, const int32_t *d, int32_t *hist, const PL &dst)
{
  for (int c = 0; c < p.out_ch; c++)
    aconv_shape_channel<K> (p, v + (size_t) c * dst.frames, d + (size_t) c * dst.frames, hist, aconv_plane_ptr (dst, c), dst.frames, 0);
}

template <int K> GSTAMD_AC void aconv_shape_planes (const AConvPlan &p, const int32_t *v, const int32_t *d, int32_t *hist, const AConvPlanes &dst)
{
  aconv_shape_planes_of<K> (p, v, d, hist, dst);
}

// head[] of a launch's rows (host).  rows_are_planes: row y works on plane y alone (the second kernel; the first one without a mix);
// otherwise every row reads all the planes: where they reach a dword boundary at the same frame the four-frame lanes start there, where they
// do not (1- to 3-byte samples in planes of different phase) the lanes realign what they load.
inline void aconv_planes_heads (AConvPlanes *pl, int planes, int rows, int bytes, bool grouped, bool rows_are_planes)
{
  uint8_t h[GSTAMD_AUDIO_MAX_CHANNELS];
  bool same = true;
  for (int c = 0; c < planes; c++) {
    const AConvSplit s = aconv_split (pl->p[c], bytes, pl->frames, grouped);
    h[c] = s.groups ? (uint8_t) s.head : 4;
    same = same && h[c] == h[0];
  }
  for (int y = 0; y < GSTAMD_AUDIO_MAX_CHANNELS; y++)
    pl->head[y] = y >= rows ? 4 : rows_are_planes ? h[y] : (same ? h[0] : 4);
  pl->realign = grouped && !rows_are_planes && !same && bytes < 4 && pl->frames >= 12 ? 1 : 0;
}

// lanes of the longest row
inline size_t aconv_planes_lanes (const AConvPlanes &pl, int rows)
{
  size_t m = 0;
  for (int y = 0; y < rows; y++) {
    const size_t l = aconv_split_lanes (aconv_plane_split (pl, y));
    m = l > m ? l : m;
  }
  return m;
}

// four-frame lanes on a non-interleaved input also serve the mixer (which a layout change always runs)
GSTAMD_AC bool aconv_pre_grouped_planes (const AConvPlan &p) { return p.mid_in == AMID_S32 || p.mid_in == AMID_F64; }
// ... and on interleaved frames whose layout changes (aconv_pre_lane_mix; the mixer between two interleaved sides keeps its lane per sample)
GSTAMD_AC bool aconv_pre_grouped_mix (const AConvPlan &p) { return p.mix && (p.mid_in == AMID_S32 || p.mid_in == AMID_F64); }

// ---- the wide converter's mixing first kernel (1 .. 64 channels) -------------------------------------------------------
// A workgroup takes a tile of frames.  Phase 1 (aconv_wide_stage_lane, aconv_wide_stage_matrix): every input sample of the tile is unpacked
// ONCE into LDS, in the mid_in format - x[frame][channel], 4-byte slots (S16 widened, S32, F32) or 8-byte ones (F64), rows of in_ch | 1
// slots - and the matrix (mi for the integer formats, m for the float ones: 4-byte entries either way) is copied beside it as it lies in
// device memory, [in][out] with rows of out_ch.  Phase 2 after the barrier (aconv_wide_mix_lane): lane -> (frame, output channel), the
// output channel running fastest, and the sums of aconv_pre_sample_at: input channels ascending, one accumulator from zero, the product
// rounded and then added, only the channels of use[co].  What the lanes of a wave read then is one x slot broadcast (or, with few output
// channels, rows in_ch | 1 slots apart: an odd stride meets every bank once) and consecutive matrix entries.
struct AConvWideMatrix {        // device memory, owned by the converter
  const float *m;               // [in][out], row stride out_ch
  const int32_t *mi;
  const uint64_t *use;          // [out]: bit ci = input channel ci takes part
};

typedef uint64_t __attribute__ ((may_alias)) aconv_u64;
typedef uint16_t __attribute__ ((may_alias)) aconv_u16;

// frames of a tile: about 2048 samples of the wider side, a multiple of four (so every tile starts at the buffer's byte phase), 32 .. 256
GSTAMD_AC int aconv_wide_tile_frames (int in_ch, int out_ch)
{
  const int t = (2048 / (in_ch > out_ch ? in_ch : out_ch)) & ~3;
  return t < 32 ? 32 : (t > 256 ? 256 : t);
}
GSTAMD_AC int aconv_wide_x_stride (const AConvPlan &p) { return p.in_ch | 1; }
GSTAMD_AC size_t aconv_wide_x_bytes (const AConvPlan &p, int tile) { return (size_t) (p.mid_in == AMID_F64 ? 8 : 4) * (size_t) tile * (size_t) aconv_wide_x_stride (p); }
GSTAMD_AC size_t aconv_wide_lds_bytes (const AConvPlan &p, int tile) { return aconv_wide_x_bytes (p, tile) + (p.mix ? 4 * (size_t) p.in_ch * (size_t) p.out_ch : 0); }

// aconv_split for a run of n samples inside a tile, on the device
GSTAMD_AC AConvSplit aconv_wide_split (const uint8_t *q, int bytes, size_t n)
{
  AConvSplit s = { 0, 0, n };
  size_t h = 0;
  while (h < 4 && (((uintptr_t) q + (size_t) bytes * h) & 3u))
    h++;
  if (h == 4 || n < h + 4)
    return s;
  s.head = h;
  s.groups = (n - h) / 4;
  return s;
}

GSTAMD_AC void aconv_wide_put32 (uint8_t *x, size_t e, uint32_t v) { ((aconv_u32 *) x)[e] = v; }
GSTAMD_AC void aconv_wide_put64 (uint8_t *x, size_t e, uint64_t v) { ((aconv_u64 *) x)[e] = v; }

// one sample at q into slot e
template <int K> GSTAMD_AC void aconv_wide_stage1 (const AConvPlan &p, const uint8_t *q, uint8_t *x, size_t e)
{
  switch (p.mid_in) {
    case AMID_S16: {
      int16_t v; memcpy (&v, q, 2);
      aconv_wide_put32 (x, e, (uint32_t) (int32_t) v);
      break;
    }
    case AMID_S32: aconv_wide_put32 (x, e, (uint32_t) aconv_unpack_int<K> (p, q, 0)); break;
    case AMID_F32: {
      uint32_t v; memcpy (&v, q, 4);
      aconv_wide_put32 (x, e, v);
      break;
    }
    default:
      aconv_wide_put64 (x, e, d_bits (p.convert_in ? aconv_s32_to_double (aconv_unpack_int<K> (p, q, 0)) : aconv_unpack_flt<K> (q, 0)));
      break;
  }
}

// four consecutive samples on aligned dwords at q into the slots e[0 .. 3]
template <int K> GSTAMD_AC void aconv_wide_stage4 (const AConvPlan &p, const uint8_t *q, uint8_t *x, const size_t e[4])
{
  if (p.mid_in == AMID_F64) {
    double r[4];
    aconv_unpack4_f64<K> (p, q, r);
    for (int j = 0; j < 4; j++)
      aconv_wide_put64 (x, e[j], d_bits (r[j]));
    return;
  }
  if constexpr (akind_bytes (K) <= 4) {
    uint32_t w[4];
    aconv_load4<K> (q, w);
    for (int j = 0; j < 4; j++)
      aconv_wide_put32 (x, e[j], p.mid_in == AMID_S32 ? (uint32_t) aconv_w_to_s32 (p, w[j]) : p.mid_in == AMID_S16 ? (uint32_t) (int32_t) (int16_t) w[j] : w[j]);
  }
}

// phase 1: the tile's frames n0 .. n0 + nf - 1 into x.  in_planar: src.p[ci] are the planes, otherwise src.p[0] holds interleaved frames.
// A run - the tile's samples of a plane, or all of them for interleaved frames - is split like a launch of the unmixed kernels: single
// samples up to the first dword a sample starts on, lanes of four samples on aligned dwords, single ones again.
template <int K, class PL> GSTAMD_AC void aconv_wide_stage_lane (const AConvPlan &p, const PL &src, int in_planar, size_t n0, int nf, uint8_t *x, int tid, int nthreads)
{
  constexpr int B = akind_bytes (K);
  const size_t xs = (size_t) aconv_wide_x_stride (p), ich = (size_t) p.in_ch;
  const size_t runs = in_planar ? ich : 1, count = in_planar ? (size_t) nf : (size_t) nf * ich;
  for (size_t t = (size_t) tid; t < runs * count; t += (size_t) nthreads) {
    const size_t b = t / count, k = t % count;
    const uint8_t *base = in_planar ? aconv_plane_ptr (src, (int) b) + (size_t) B * n0 : aconv_plane_ptr (src, 0) + (size_t) B * n0 * ich;
    const AConvSplit s = aconv_wide_split (base, B, count);
    if (k >= aconv_split_lanes (s))
      continue;
    if (k >= s.groups) {
      const size_t i = aconv_split_single (s, k);
      aconv_wide_stage1<K> (p, base + (size_t) B * i, x, in_planar ? i * xs + b : (i / ich) * xs + i % ich);
      continue;
    }
    const size_t i = s.head + 4 * k;
    size_t e[4];
    for (int j = 0; j < 4; j++)
      e[j] = in_planar ? (i + (size_t) j) * xs + b : ((i + (size_t) j) / ich) * xs + (i + (size_t) j) % ich;
    aconv_wide_stage4<K> (p, base + (size_t) B * i, x, e);
  }
}

// the matrix the mixer of this plan reads, as dwords
GSTAMD_AC const uint32_t *aconv_wide_matrix_of (const AConvPlan &p, const AConvWideMatrix &w)
{
  return p.mid_in == AMID_S16 || p.mid_in == AMID_S32 ? (const uint32_t *) w.mi : (const uint32_t *) w.m;
}

GSTAMD_AC void aconv_wide_stage_matrix (const AConvPlan &p, const AConvWideMatrix &w, uint8_t *mat, int tid, int nthreads)
{
  const aconv_u32 *src = (const aconv_u32 *) aconv_wide_matrix_of (p, w);
  for (int i = tid; i < p.in_ch * p.out_ch; i += nthreads)
    aconv_wide_put32 (mat, (size_t) i, src[i]);
}

// phase 2: (frame f, output channel co) of the tile -> the interleaved mid buffer
GSTAMD_AC void aconv_wide_mix_lane (const AConvPlan &p, const uint8_t *x, const uint8_t *mat, const uint64_t *use_of, uint8_t *mid, size_t n0, int nf, int tid, int nthreads)
{
  const size_t xs = (size_t) aconv_wide_x_stride (p), och = (size_t) p.out_ch;
  const aconv_u32 *mw = (const aconv_u32 *) mat;
  for (size_t o = (size_t) tid; o < (size_t) nf * och; o += (size_t) nthreads) {
    const size_t f = o / och, co = o % och, oi = (n0 + f) * och + co;
    const aconv_u32 *x4 = (const aconv_u32 *) x + f * xs;
    const aconv_u64 *x8 = (const aconv_u64 *) x + f * xs;
    const uint64_t use = p.mix ? use_of[co] : 0;
    switch (p.mid_in) {
      case AMID_S16: {
        int32_t res;
        if (!p.mix) {
          res = (int32_t) x4[co];
        } else {
          uint32_t acc = 0;                     /* the reference's gint32, which wraps */
          for (int ci = 0; ci < p.in_ch; ci++)
            if ((use >> ci) & 1u)
              acc += x4[ci] * mw[(size_t) ci * och + co];
          res = (int32_t) (acc + 512u) >> 10;
          res = res > 32767 ? 32767 : (res < -32768 ? -32768 : res);
        }
        ((aconv_u16 *) mid)[oi] = (uint16_t) (int16_t) res;
        break;
      }
      case AMID_S32: {
        int32_t r;
        if (!p.mix) {
          r = (int32_t) x4[co];
        } else {
          int64_t res = 0;
          for (int ci = 0; ci < p.in_ch; ci++)
            if ((use >> ci) & 1u)
              res += (int64_t) (int32_t) x4[ci] * (int64_t) (int32_t) mw[(size_t) ci * och + co];
          r = aconv_mix_round_s32 (res);
        }
        ((aconv_u32 *) mid)[oi] = (uint32_t) r;
        break;
      }
      case AMID_F32: {
        uint32_t rw;
        if (!p.mix) {
          rw = x4[co];
        } else {
          float r = 0.0f;
          for (int ci = 0; ci < p.in_ch; ci++)
            if ((use >> ci) & 1u)
              r += bits_f (x4[ci]) * bits_f (mw[(size_t) ci * och + co]);
          rw = f_bits (r);
        }
        ((aconv_u32 *) mid)[oi] = rw;
        break;
      }
      default: {
        uint64_t rw;
        if (!p.mix) {
          rw = x8[co];
        } else {
          double r = 0.0;
          for (int ci = 0; ci < p.in_ch; ci++)
            if ((use >> ci) & 1u)
              r += bits_d (x8[ci]) * bits_f (mw[(size_t) ci * och + co]);
          rw = d_bits (r);
        }
        ((aconv_u64 *) mid)[oi] = rw;
        break;
      }
    }
  }
}

// head[] of the rows of a wide second kernel (host): row y writes plane y alone
inline void aconv_planes_heads_wide (AConvPlanesWide *pl, int planes, int bytes, bool grouped)
{
  for (int y = 0; y < GSTAMD_AUDIO_MAX_CHANNELS_WIDE; y++) {
    const AConvSplit s = y < planes ? aconv_split (pl->p[y], bytes, pl->frames, grouped) : AConvSplit { 0, 0, 0 };
    pl->head[y] = s.groups ? (uint8_t) s.head : 4;
  }
  pl->realign = 0;
}

inline size_t aconv_planes_lanes_wide (const AConvPlanesWide &pl, int rows)
{
  size_t m = 0;
  for (int y = 0; y < rows; y++) {
    const size_t l = aconv_split_lanes (aconv_plane_split_of (pl, y));
    m = l > m ? l : m;
  }
  return m;
}

// ---- the endian plan (converter_endian): every sample's bytes reversed, nothing else.  K is the little-endian container of the width;
// reading it as LE and writing it as BE is the swap in either direction.  in == out is fine: a lane reads its bytes before it writes them.
template <int K> GSTAMD_AC void aconv_swap_lane (const uint8_t *in, uint8_t *out, const AConvSplit &s, size_t t)
{
  constexpr int B = akind_bytes (K);
  if (t >= s.groups) {
    const size_t i = aconv_split_single (s, t);
    if constexpr (B == 8)
      aconv_store_w64<K + 1> (out, i, aconv_load_w64<K> (in, i));
    else
      aconv_store_w<K + 1> (out, i, aconv_load_w<K> (in, i));
    return;
  }
  const size_t i = s.head + 4 * t;
  if constexpr (B == 8) {
    uint64_t w[4];
    aconv_load4_64<K> (in + 8 * i, w);
    aconv_store4_64<K + 1> (out + 8 * i, w);
  } else {
    uint32_t w[4];
    aconv_load4<K> (in + (size_t) B * i, w);
    aconv_store4<K + 1> (out + (size_t) B * i, w);
  }
}

// the lanes of a swap: grouped where the two buffers reach a dword boundary at the same sample
inline AConvSplit aconv_swap_split (const void *in, const void *out, int bytes, size_t n)
{
  return aconv_split (in, bytes, n, (((uintptr_t) in ^ (uintptr_t) out) & 3u) == 0);
}

// ---- many converters of one plan in one set of launches (gstamd_audio_converter_samples_many) --------------------------
// blockIdx.y (for the shaping kernel blockIdx.x) is the stream.  What differs between two streams of a plan - buffers, how the lanes share
// them, where the dither generator stands - comes by value in the kernel arguments, one table per kernel, read with an index that is
// uniform over the workgroup.  64 entries have to fit 4 KB beside the 664 bytes of the plan, so an entry holds no more than its kernel
// needs: an AConvSplit is packed into eight bytes, and a stream's dither words follow its samples in one buffer (q, q + n).
#define GSTAMD_ACONV_MANY_MAX 64

struct AConvSplitPacked {
  uint64_t v;                   // bits 0 .. 39: n (a stream of a run has fewer than 2^30 frames of at most 8 channels); 40 .. 41: head; 42: grouped
};

GSTAMD_AC AConvSplitPacked aconv_split_pack (const AConvSplit &s)
{
  return { (uint64_t) s.n | ((uint64_t) s.head << 40) | ((uint64_t) (s.groups ? 1 : 0) << 42) };
}

GSTAMD_AC AConvSplit aconv_split_unpack (AConvSplitPacked k)
{
  AConvSplit s = { 0, 0, (size_t) (k.v & 0xffffffffffull) };
  if ((k.v >> 42) & 1u) {
    s.head = (size_t) ((k.v >> 40) & 3u);
    s.groups = (s.n - s.head) / 4;
  }
  return s;
}

struct AConvManyPre {           // 24 bytes
  const uint8_t *in;
  uint8_t *mid;
  AConvSplitPacked split;
};

struct AConvManyPost {          // 48 bytes
  const uint8_t *mid;
  uint8_t *out;
  int32_t *q;                   // with noise shaping: split.n S32 samples, then as many dither words
  AConvSplitPacked split;       // n == 0: the resampler only took history - no lanes, no draws
  AConvDitherState ds;
  int pad;
};

struct AConvManyShape {         // 32 bytes
  const int32_t *q;
  int32_t *hist;
  uint8_t *out;
  size_t frames;
};

struct AConvManyPreTable { AConvManyPre s[GSTAMD_ACONV_MANY_MAX]; };
struct AConvManyPostTable { AConvManyPost s[GSTAMD_ACONV_MANY_MAX]; };
struct AConvManyShapeTable { AConvManyShape s[GSTAMD_ACONV_MANY_MAX]; };
static_assert (sizeof (AConvManyPre) == 24 && sizeof (AConvManyPost) == 48 && sizeof (AConvManyShape) == 32, "entries of the tables");
static_assert (sizeof (AConvPlan) + sizeof (void *) + sizeof (AConvManyPostTable) <= 3840, "kernel arguments end at 4 KB");

// lane t of stream m: the lane of the stream's own k_aconv_pre / k_aconv_post launch; lanes past a shorter stream's end do nothing
template <int K> GSTAMD_AC void aconv_pre_many_lane (const AConvPlan &p, const AConvManyPre &m, size_t t)
{
  const AConvSplit s = aconv_split_unpack (m.split);
  if (t >= aconv_split_lanes (s))
    return;
  aconv_pre_lane<K> (p, m.in, m.mid, s, t);
}

template <int K> GSTAMD_AC void aconv_post_many_lane (const AConvPlan &p, const AConvJump &jump, const AConvManyPost &m, size_t t)
{
  const AConvSplit s = aconv_split_unpack (m.split);
  if (t >= aconv_split_lanes (s))
    return;
  aconv_post_lane<K> (p, jump, m.ds, m.mid, m.out, m.q, m.q ? m.q + s.n : nullptr, s, t);
}

// lane c of stream m's 64-lane workgroup: one channel's error recurrence, all streams' channels side by side
template <int K> GSTAMD_AC void aconv_shape_many_lane (const AConvPlan &p, const AConvManyShape &m, int c)
{
  if (c < p.out_ch && m.frames)
    aconv_shape_channel<K> (p, m.q, m.q + m.frames * (size_t) p.out_ch, m.hist, m.out, m.frames, c);
}

// ---- the same for converters with a non-interleaved side and for wide ones ----------------------------------------------
// gstamd_audio_converter_samples_many takes what gstamd_audio_converter_samples takes: a non-interleaved side is ONE pointer with the planes
// frames * bytes apart.  So a side is 16 bytes whatever its channel count, and the lane bodies of a non-interleaved side run on an
// AConvPlanesEven made from it in registers; the 88 and 592 bytes of AConvPlanes / AConvPlanesWide would not fit 64 times.
struct AConvManySide {          // 16 bytes
  uint8_t *base;
  uint32_t frames;              // fewer than 2^30
  uint32_t how;                 // bits 0 .. 2: AConvPlanesEven::how; bit 3: realign
};

GSTAMD_AC AConvPlanesEven aconv_many_side (const AConvManySide &e, int bytes)
{
  return { e.base, (size_t) e.frames, bytes, (int) (e.how & 7u), (int) ((e.how >> 3) & 1u) };
}

struct AConvManyPrePlanes {     // 24 bytes: k_aconv_pre_planes_many, k_aconv_wide_mix_many (which looks at no head)
  AConvManySide in;
  uint8_t *mid;
};

struct AConvManyPostPlanes {    // 48 bytes
  const uint8_t *mid;
  int32_t *q;                   // with noise shaping: frames * out_ch S32 samples in the quantizer's order, then as many dither words
  AConvManySide out;            // frames == 0: the resampler only took history - no lanes, no draws
  AConvDitherState ds;
  int pad;
};

struct AConvManyPrePlanesTable { AConvManyPrePlanes s[GSTAMD_ACONV_MANY_MAX]; };
struct AConvManyPostPlanesTable { AConvManyPostPlanes s[GSTAMD_ACONV_MANY_MAX]; };
static_assert (sizeof (AConvManySide) == 16 && sizeof (AConvManyPrePlanes) == 24 && sizeof (AConvManyPostPlanes) == 48, "entries of the tables");
static_assert (sizeof (AConvPlan) + sizeof (void *) + sizeof (AConvManyPostPlanesTable) <= 3840, "kernel arguments end at 4 KB");
static_assert (sizeof (AConvPlan) + sizeof (AConvWideMatrix) + sizeof (AConvManyPrePlanesTable) + 2 * sizeof (int) <= 3840, "kernel arguments end at 4 KB");

// lane t of row co (an output channel) of stream m: the lane of the stream's own k_aconv_pre_planes / k_aconv_pre_mix launch
template <int K> GSTAMD_AC void aconv_pre_planes_many_lane (const AConvPlan &p, const AConvManyPrePlanes &m, int co, size_t t)
{
  aconv_pre_lane_planes_of<K> (p, aconv_many_side (m.in, akind_bytes (K)), m.mid, co, t);
}

template <int K> GSTAMD_AC void aconv_pre_mix_many_lane (const AConvPlan &p, const AConvManyPre &m, int co, size_t t)
{
  aconv_pre_lane_mix<K> (p, m.in, m.mid, aconv_split_unpack (m.split), co, t);          /* m.split: of the stream's FRAMES */
}

// lane t of output plane c of stream m: k_aconv_post_planes / k_aconv_wide_post_planes
template <int K> GSTAMD_AC void aconv_post_planes_many_lane (const AConvPlan &p, const AConvJump &jump, const AConvManyPostPlanes &m, int c, size_t t)
{
  const size_t n = (size_t) m.out.frames * (size_t) p.out_ch;
  aconv_post_lane_planes_of<K> (p, jump, m.ds, m.mid, aconv_many_side (m.out, akind_bytes (K)), m.q, m.q ? m.q + n : nullptr, c, t);
}

// stream m's one recurrence over plane 0, plane 1, ... (k_aconv_shape_planes / k_aconv_wide_shape_planes); the caller gives every lane
// of a wave another stream
template <int K> GSTAMD_AC void aconv_shape_planes_many_lane (const AConvPlan &p, const AConvManyShape &m)
{
  if (m.frames && m.q)
    aconv_shape_planes_of<K> (p, m.q, m.q + m.frames * (size_t) p.out_ch, m.hist, AConvPlanesEven { m.out, m.frames, akind_bytes (K), 4, 0 });
}

// the workgroup of k_aconv_wide_mix_many for tile `tile_index` of stream m; false: the stream has no such tile and the workgroup leaves
// (as a whole, before the barrier).  n0 / nf: the tile's first frame and its frames.
GSTAMD_AC bool aconv_wide_many_tile (const AConvManyPrePlanes &m, size_t tile_index, int tile, size_t *n0, int *nf)
{
  *n0 = tile_index * (size_t) tile;
  if (*n0 >= (size_t) m.in.frames)
    return false;
  *nf = (size_t) m.in.frames - *n0 < (size_t) tile ? (int) ((size_t) m.in.frames - *n0) : tile;
  return true;
}

#ifndef __HIPCC__
// ---- one sample at a time with the container looked up per call: the entry points of a host loop that walks samples, not lanes
// (tests/emu/emu_audio.cpp).  The kernels never come here.  For the endian plan the first stage parks the container in the sample's mid
// slot (which is at least as wide) and the second one writes it out reversed.
inline void aconv_pre_sample (const AConvPlan &p, const uint8_t *in, uint8_t *mid, size_t n, int co)
{
  if (p.endian_swap) {
    const size_t i = n * (size_t) p.out_ch + (size_t) co;
    memcpy (mid + (size_t) amid_bytes (p.mid_in) * i, in + (size_t) p.endian_swap * i, (size_t) p.endian_swap);
    return;
  }
#define GSTAMD_ACONV_F(K) aconv_pre_sample<K> (p, in, mid, n, co)
  GSTAMD_ACONV_FOR_KIND (p.in_kind, GSTAMD_ACONV_F);
#undef GSTAMD_ACONV_F
}

inline void aconv_post_sample (const AConvPlan &p, const AConvJump &jump, const AConvDitherState &ds, const uint8_t *mid, uint8_t *out, int32_t *qv, int32_t *qd, size_t i)
{
  if (p.endian_swap) {
    const uint8_t *q = mid + (size_t) amid_bytes (p.mid_in) * i;
    for (int b = 0; b < p.endian_swap; b++)
      out[(size_t) p.endian_swap * i + (size_t) b] = q[p.endian_swap - 1 - b];
    return;
  }
#define GSTAMD_ACONV_F(K) aconv_post_sample<K> (p, jump, ds, mid, out, qv, qd, i)
  GSTAMD_ACONV_FOR_KIND (p.out_kind, GSTAMD_ACONV_F);
#undef GSTAMD_ACONV_F
}

inline void aconv_shape_channel (const AConvPlan &p, const int32_t *v, const int32_t *d, int32_t *hist, uint8_t *out, size_t frames, int c)
{
#define GSTAMD_ACONV_F(K) aconv_shape_channel<K> (p, v, d, hist, out, frames, c)
  GSTAMD_ACONV_FOR_KIND (p.out_kind, GSTAMD_ACONV_F);
#undef GSTAMD_ACONV_F
}
#endif

}  // namespace gstamd
