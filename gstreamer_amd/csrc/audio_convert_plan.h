// audio_convert_plan.h - the decision code of gst_audio_converter_new (audio-converter.c:1346-1470) restated: which stages a conversion
// has and on which intermediate format they run.  Host only; shared by audio_convert.hip and the host emulation of tests/emu.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gstamd_video.h"
#include "audio_convert_device.h"

// ---- the plan: gst_audio_converter_new's chain ---------------------------------------------------------------------------------------
namespace gstamd {

struct AFmtInfo {
  bool known, integer;
  int depth;
};

static AFmtInfo afmt_info (int fmt)
{
  const AFmtDesc d = afmt_desc (fmt);
  return {d.known, d.integer, d.depth};
}

// the same format apart from the byte order (S16LE / S16BE, U20LE / U20BE, F64LE / F64BE ...)
static bool afmt_endian_pair (int a, int b)
{
  const AFmtDesc x = afmt_desc (a), y = afmt_desc (b);
  return x.known && y.known && x.integer == y.integer && x.usgn == y.usgn && x.depth == y.depth && x.bytes == y.bytes && x.be != y.be;
}

static bool afmt_is_intermediate (int fmt)
{
  return fmt == GSTAMD_AFMT_S16LE || fmt == GSTAMD_AFMT_S32LE || fmt == GSTAMD_AFMT_F32LE || fmt == GSTAMD_AFMT_F64LE;
}

static int afmt_mid (int fmt)
{
  return fmt == GSTAMD_AFMT_S16LE ? AMID_S16 : fmt == GSTAMD_AFMT_S32LE ? AMID_S32 : fmt == GSTAMD_AFMT_F32LE ? AMID_F32 : AMID_F64;
}

// ---- the default mixing matrix: gst_audio_channel_mixer_fill_matrix (audio-channel-mixer.c:731-805) restated --------------------------
// Positions are GstAudioChannelPosition values (audio-channels.h:101-133).
enum APos : int {
  APOS_NONE = -3, APOS_MONO = -2, APOS_INVALID = -1, APOS_FL = 0, APOS_FR = 1, APOS_FC = 2, APOS_LFE1 = 3, APOS_RL = 4, APOS_RR = 5, APOS_FLOC = 6, APOS_FROC = 7,
  APOS_RC = 8, APOS_LFE2 = 9, APOS_SL = 10, APOS_SR = 11
};

// The matrices are flat [in][out] arrays with a row stride `ms`: 8 inside an AConvPlan, the output channel count in a wide plan.

// fill_compatible (:163-253): mono <-> stereo pairs of the front, the centre pair and the rear
static void amix_fill_compatible (float *m, int ms, int in_ch, const int *ip, int out_ch, const int *op)
{
  auto M = [&](int i, int j) -> float & { return m[i * ms + j]; };
  static const int conv[3][3] = { {APOS_FL, APOS_FR, APOS_MONO}, {APOS_FLOC, APOS_FROC, APOS_FC}, {APOS_RL, APOS_RR, APOS_RC} };
  for (int c = 0; c < 3; c++) {
    int a0 = -1, a1 = -1, a2 = -1, b0 = -1, b1 = -1, b2 = -1;
    for (int n = 0; n < in_ch; n++) {
      if (ip[n] == conv[c][0]) a0 = n;
      else if (ip[n] == conv[c][1]) a1 = n;
      else if (ip[n] == conv[c][2]) a2 = n;
    }
    for (int n = 0; n < out_ch; n++) {
      if (op[n] == conv[c][0]) b0 = n;
      else if (op[n] == conv[c][1]) b1 = n;
      else if (op[n] == conv[c][2]) b2 = n;
    }
    /* left -> centre, right -> centre */
    if (a0 != -1 && a2 == -1 && b0 == -1 && b2 != -1) M (a0, b2) = 1.0f;
    else if (a0 != -1 && a2 != -1 && b0 == -1 && b2 != -1) M (a0, b2) = 0.5f;
    else if (a0 != -1 && a2 == -1 && b0 != -1 && b2 != -1) M (a0, b2) = 1.0f;
    if (a1 != -1 && a2 == -1 && b1 == -1 && b2 != -1) M (a1, b2) = 1.0f;
    else if (a1 != -1 && a2 != -1 && b1 == -1 && b2 != -1) M (a1, b2) = 0.5f;
    else if (a1 != -1 && a2 == -1 && b1 != -1 && b2 != -1) M (a1, b2) = 1.0f;
    /* centre -> left, centre -> right */
    if (a2 != -1 && a0 == -1 && b2 == -1 && b0 != -1) M (a2, b0) = 1.0f;
    else if (a2 != -1 && a0 != -1 && b2 == -1 && b0 != -1) M (a2, b0) = 0.5f;
    else if (a2 != -1 && a0 == -1 && b2 != -1 && b0 != -1) M (a2, b0) = 1.0f;
    if (a2 != -1 && a1 == -1 && b2 == -1 && b1 != -1) M (a2, b1) = 1.0f;
    else if (a2 != -1 && a1 != -1 && b2 == -1 && b1 != -1) M (a2, b1) = 0.5f;
    else if (a2 != -1 && a1 == -1 && b2 != -1 && b1 != -1) M (a2, b1) = 1.0f;
  }
}

struct AMixGroups {             // detect_pos (:264-327): [0] left, [1] centre-ish, [2] right of the five families
  int f[3] = { -1, -1, -1 }, c[3] = { -1, -1, -1 }, r[3] = { -1, -1, -1 }, s[3] = { -1, -1, -1 }, b[3] = { -1, -1, -1 };
  bool has_f = false, has_c = false, has_r = false, has_s = false, has_b = false;
};

static void amix_detect (int ch, const int *pos, AMixGroups &g)
{
  for (int n = 0; n < ch; n++)
    switch (pos[n]) {
      case APOS_MONO: g.f[1] = n; g.has_f = true; break;
      case APOS_FL: g.f[0] = n; g.has_f = true; break;
      case APOS_FR: g.f[2] = n; g.has_f = true; break;
      case APOS_FC: g.c[1] = n; g.has_c = true; break;
      case APOS_FLOC: g.c[0] = n; g.has_c = true; break;
      case APOS_FROC: g.c[2] = n; g.has_c = true; break;
      case APOS_RC: g.r[1] = n; g.has_r = true; break;
      case APOS_RL: g.r[0] = n; g.has_r = true; break;
      case APOS_RR: g.r[2] = n; g.has_r = true; break;
      case APOS_SL: g.s[0] = n; g.has_s = true; break;
      case APOS_SR: g.s[2] = n; g.has_s = true; break;
      case APOS_LFE1: g.b[1] = n; g.has_b = true; break;
      default: break;
    }
}

// fill_one_other (:329-378); `ratio` is a gfloat there and 0.5 * ratio is rounded to float on the store
static void amix_one_other (float *m, int ms, const int *from, const int *to, float ratio)
{
  const float half = (float) (0.5 * (double) ratio);
  auto M = [&](int i, int j) -> float & { return m[i * ms + j]; };
  if (from[1] != -1 && to[1] != -1) M (from[1], to[1]) = ratio;
  if (from[0] != -1 && to[0] != -1) M (from[0], to[0]) = ratio;
  if (from[2] != -1 && to[2] != -1) M (from[2], to[2]) = ratio;
  if (from[0] != -1 && to[1] != -1) M (from[0], to[1]) = from[1] != -1 ? half : ratio;
  if (from[2] != -1 && to[1] != -1) M (from[2], to[1]) = from[1] != -1 ? half : ratio;
  if (from[1] != -1 && to[0] != -1) M (from[1], to[0]) = from[0] != -1 ? half : ratio;
  if (from[1] != -1 && to[2] != -1) M (from[1], to[2]) = from[2] != -1 ? half : ratio;
}

// fill_others (:398-590): a family one side lacks goes to / comes from the nearest family the other side has
static void amix_fill_others (float *m, int ms, int in_ch, const int *ip, int out_ch, const int *op)
{
  AMixGroups i, o;
  amix_detect (in_ch, ip, i);
  amix_detect (out_ch, op, o);
  const double R2 = 1.0 / sqrt (2.0), R8 = 1.0 / sqrt (8.0);
  const double CENTER_FRONT = R2, CENTER_SIDE = 0.5, CENTER_REAR = R8, FRONT_SIDE = R2, FRONT_REAR = 0.5, SIDE_REAR = R2;
  const double CENTER_BASS = R2, FRONT_BASS = 1.0, SIDE_BASS = R2, REAR_BASS = R2;
  auto go = [&](const int *from, const int *to, double ratio) { amix_one_other (m, ms, from, to, (float) ratio); };
  /* centre <-> front / side / rear */
  if (!i.has_c && i.has_f && o.has_c) go (i.f, o.c, CENTER_FRONT);
  else if (!i.has_c && !i.has_f && i.has_s && o.has_c) go (i.s, o.c, CENTER_SIDE);
  else if (!i.has_c && !i.has_f && !i.has_s && i.has_r && o.has_c) go (i.r, o.c, CENTER_REAR);
  else if (i.has_c && !o.has_c && o.has_f) go (i.c, o.f, CENTER_FRONT);
  else if (i.has_c && !o.has_c && !o.has_f && o.has_s) go (i.c, o.s, CENTER_SIDE);
  else if (i.has_c && !o.has_c && !o.has_f && !o.has_s && o.has_r) go (i.c, o.r, CENTER_REAR);
  /* front <-> centre / side / rear */
  if (!i.has_f && i.has_c && !i.has_s && o.has_f) go (i.c, o.f, CENTER_FRONT);
  else if (!i.has_f && !i.has_c && i.has_s && o.has_f) go (i.s, o.f, FRONT_SIDE);
  else if (!i.has_f && i.has_c && i.has_s && o.has_f) { go (i.c, o.f, 0.5 * CENTER_FRONT); go (i.s, o.f, 0.5 * FRONT_SIDE); }
  else if (!i.has_f && !i.has_c && !i.has_s && i.has_r && o.has_f) go (i.r, o.f, FRONT_REAR);
  else if (i.has_f && o.has_c && !o.has_s && !o.has_f) go (i.f, o.c, CENTER_FRONT);
  else if (i.has_f && !o.has_c && o.has_s && !o.has_f) go (i.f, o.s, FRONT_SIDE);
  else if (i.has_f && o.has_c && o.has_s && !o.has_f) { go (i.f, o.c, 0.5 * CENTER_FRONT); go (i.f, o.s, 0.5 * FRONT_SIDE); }
  else if (i.has_f && !o.has_c && !o.has_s && !o.has_f && o.has_r) go (i.f, o.r, FRONT_REAR);
  /* side <-> centre / front / rear */
  if (!i.has_s && i.has_f && !i.has_r && o.has_s) go (i.f, o.s, FRONT_SIDE);
  else if (!i.has_s && !i.has_f && i.has_r && o.has_s) go (i.r, o.s, SIDE_REAR);
  else if (!i.has_s && i.has_f && i.has_r && o.has_s) { go (i.f, o.s, 0.5 * FRONT_SIDE); go (i.r, o.s, 0.5 * SIDE_REAR); }
  else if (!i.has_s && !i.has_f && !i.has_r && i.has_c && o.has_s) go (i.c, o.s, CENTER_SIDE);
  else if (i.has_s && o.has_f && !o.has_r && !o.has_s) go (i.s, o.f, FRONT_SIDE);
  else if (i.has_s && !o.has_f && o.has_r && !o.has_s) go (i.s, o.r, SIDE_REAR);
  else if (i.has_s && o.has_f && o.has_r && !o.has_s) { go (i.s, o.f, 0.5 * FRONT_SIDE); go (i.s, o.r, 0.5 * SIDE_REAR); }
  else if (i.has_s && !o.has_f && !o.has_r && o.has_c && !o.has_s) go (i.s, o.c, CENTER_SIDE);
  /* rear <-> centre / front / side */
  if (!i.has_r && i.has_s && o.has_r) go (i.s, o.r, SIDE_REAR);
  else if (!i.has_r && !i.has_s && i.has_f && o.has_r) go (i.f, o.r, FRONT_REAR);
  else if (!i.has_r && !i.has_s && !i.has_f && i.has_c && o.has_r) go (i.c, o.r, CENTER_REAR);
  else if (i.has_r && !o.has_r && o.has_s) go (i.r, o.s, SIDE_REAR);
  else if (i.has_r && !o.has_r && !o.has_s && o.has_f) go (i.r, o.f, FRONT_REAR);
  else if (i.has_r && !o.has_r && !o.has_s && !o.has_f && o.has_c) go (i.r, o.c, CENTER_REAR);
  /* bass <-> any */
  if (i.has_b && !o.has_b) {
    if (o.has_c) go (i.b, o.c, CENTER_BASS);
    if (o.has_f) go (i.b, o.f, FRONT_BASS);
    if (o.has_s) go (i.b, o.s, SIDE_BASS);
    if (o.has_r) go (i.b, o.r, REAR_BASS);
  } else if (!i.has_b && o.has_b) {
    if (i.has_c) go (i.c, o.b, CENTER_BASS);
    if (i.has_f) go (i.f, o.b, FRONT_BASS);
    if (i.has_s) go (i.s, o.b, REAR_BASS);              /* the reference uses the rear ratio for the sides here (:581) */
    if (i.has_r) go (i.r, o.b, REAR_BASS);
  }
}

// fill_normalize (:596-626): float sums of |m| per output channel, every entry divided by the largest
static void amix_normalize (float *m, int ms, int in_ch, int out_ch)
{
  auto M = [&](int i, int j) -> float & { return m[i * ms + j]; };
  float top = 0;
  for (int j = 0; j < out_ch; j++) {
    float sum = 0.0f;
    for (int i = 0; i < in_ch; i++)
      sum = (float) ((double) sum + fabs ((double) M (i, j)));
    if (sum > top)
      top = sum;
  }
  if (top == 0.0f)
    return;
  for (int j = 0; j < out_ch; j++)
    for (int i = 0; i < in_ch; i++)
      M (i, j) /= top;
}

// m: in_ch rows of ms floats
static void default_mix_matrix (int in_ch, const int *ip, bool in_unpositioned, int out_ch, const int *op, float *m, int ms)
{
  memset (m, 0, sizeof (float) * (size_t) in_ch * (size_t) ms);
  auto M = [&](int i, int j) -> float & { return m[i * ms + j]; };
  /* fill_special (:628-656) */
  if (in_ch == 2 && out_ch == 1 && ((ip[0] == APOS_FL && ip[1] == APOS_FR) || (ip[0] == APOS_FR && ip[1] == APOS_FL)) && op[0] == APOS_MONO) {
    M (0, 0) = M (1, 0) = 0.5f;
    return;
  }
  if (in_ch == 1 && out_ch == 2 && ((op[0] == APOS_FL && op[1] == APOS_FR) || (op[0] == APOS_FR && op[1] == APOS_FL)) && ip[0] == APOS_MONO) {
    M (0, 0) = M (0, 1) = 1.0f;
    return;
  }
  /* virtual inputs (:684-729): all-mono inputs count as one mono channel, alternating left / right ones as one stereo pair */
  int in_size = in_ch, virt = 0;
  if (in_ch >= 2) {
    bool mono = true, alt = true;
    for (int i = 0; i < in_ch; i++) {
      mono = mono && ip[i] == APOS_MONO;
      alt = alt && ip[i] == (i & 1 ? APOS_FR : APOS_FL);
    }
    if (mono) { virt = 1; in_size = 1; }
    else if (alt && in_ch > 2) { virt = 2; in_size = 2; }
  }
  /* fill_identical (:130-155) */
  for (int co = 0; co < out_ch; co++)
    for (int ci = 0; ci < in_size; ci++) {
      if (in_unpositioned)
        M (ci, co) = ci == co ? 1.0f : 0.0f;
      else if (ip[ci] == op[co])
        M (ci, co) = 1.0f;
    }
  if (!in_unpositioned) {
    amix_fill_compatible (m, ms, in_size, ip, out_ch, op);
    amix_fill_others (m, ms, in_size, ip, out_ch, op);
    amix_normalize (m, ms, in_size, out_ch);
  }
  if (virt == 1) {
    for (int o = 0; o < out_ch; o++)
      M (0, o) /= (float) in_ch;
    for (int i = 1; i < in_ch; i++)
      memcpy (&M (i, 0), &M (0, 0), sizeof (float) * (size_t) out_ch);
  } else if (virt == 2) {
    const int right = in_ch >> 1, left = right + (in_ch % 2);
    for (int o = 0; o < out_ch; o++) {
      M (0, o) /= (float) left;
      M (1, o) /= (float) right;
    }
    for (int i = 2; i < in_ch; i++)
      memcpy (&M (i, 0), &M (i % 2, 0), sizeof (float) * (size_t) out_ch);
  }
}

// one side of a conversion as the chain decisions see it: a GstAmdAudioInfo or a GstAmdAudioInfoWide
struct AConvSide {
  int format, rate, channels, info_layout, unpositioned;
  const int *position;
};

// The whole plan.  *resample: a resampler (on p->mid_in, out->channels) sits between the two kernels; *passthrough: the bytes
// themselves; plan->endian_swap: the bytes of every sample reversed.  Returns GSTAMD_OK or an error code with *err set.
// The layouts (GstAudioLayout: 0 interleaved, 1 non-interleaved) come beside the infos, whose own `layout` stays 0:
//   - the passthrough and the endian shortcut need equal layouts; where the layouts differ the mix stage runs even with a passthrough
//     matrix (the mixer is what changes the layout), on the intermediate format the rules below give anyway;
//   - the quantizer of a non-interleaved output walks plane after plane as one channel: q_stride 1.
// The chain does not depend on the channel count: this is the plan of both constructors.  max_ch: 8 or 64.  user: the mix-matrix option,
// [out][in] with row stride us, or NULL.  m / mi: the matrices, [in][out] with row stride ms; use[out]: the channels the mixer sums.
// plan->m / mi / use are not touched here (aconv_make_plan_layouts points m / mi at them).
inline int aconv_plan_chain (int flags, const AConvSide &in, int in_layout, const AConvSide &out, int out_layout, const GstAmdAudioConverterConfig &cfg, int max_ch,
    const float *user, int us, AConvPlan *plan, float *m, int *mi, int ms, uint64_t *use, bool *resample, bool *passthrough, std::string *err)
{
  if (in_layout < 0 || in_layout > 1 || out_layout < 0 || out_layout > 1) {
    *err = "layout is 0 (interleaved) or 1 (non-interleaved)";
    return GSTAMD_ERR_INVALID;
  }
  const AFmtInfo fi = afmt_info (in.format), fo = afmt_info (out.format);
  if (!fi.known || !fo.known) {
    *err = "not a raw sample format (GstAudioFormat 2 .. 31: S8 / U8, S16 / S24_32 / S32 / S24 / S20 / S18 signed and unsigned, F32 / F64, either byte order)";
    return GSTAMD_ERR_UNSUPPORTED;
  }
  if (in.channels < 1 || out.channels < 1 || in.channels > max_ch || out.channels > max_ch) {
    *err = max_ch == GSTAMD_AUDIO_MAX_CHANNELS ? "1 .. 8 channels" : "1 .. 64 channels";
    return max_ch == GSTAMD_AUDIO_MAX_CHANNELS ? GSTAMD_ERR_UNSUPPORTED : GSTAMD_ERR_INVALID;     /* 64 is the reference's limit too */
  }
  if (in.info_layout != 0 || out.info_layout != 0) {
    *err = "GstAmdAudioInfo.layout is 0: non-interleaved layouts are the layout arguments of gstamd_audio_converter_new_layouts";
    return GSTAMD_ERR_UNSUPPORTED;
  }
  if (in.rate <= 0 || out.rate <= 0) {
    *err = "bad rate";
    return GSTAMD_ERR_INVALID;
  }
  /* gst_audio_converter_new :1370-1378 */
  if (!user && in.channels != out.channels && (in.unpositioned || out.unpositioned)) {
    *err = "unpositioned channels with different channel counts and no mix-matrix";
    return GSTAMD_ERR_INVALID;
  }
  AConvPlan &p = *plan;
  p.in_fmt = in.format;
  p.out_fmt = out.format;
  p.in_ch = in.channels;
  p.out_ch = out.channels;
  p.q_stride = out_layout ? 1 : out.channels;
  {
    const AFmtDesc di = afmt_desc (in.format), dout = afmt_desc (out.format);
    p.in_kind = afmt_kind (in.format);
    p.out_kind = afmt_kind (out.format);
    p.in_shift = di.integer ? 32 - di.depth : 0;
    p.in_sx = di.integer && di.usgn ? 0x80000000u : 0u;
    p.out_shift = dout.integer ? 32 - dout.depth : 0;
    p.out_usgn = dout.integer && dout.usgn ? 1 : 0;
  }
  /* chain_unpack :708-740 */
  const bool same_format = in.format == out.format;
  int cur = (same_format && afmt_is_intermediate (in.format)) ? afmt_mid (in.format) : (fi.integer ? AMID_S32 : AMID_F64);
  /* chain_convert_in :742-762 */
  if (fi.integer && !fo.integer) {
    p.convert_in = 1;
    cur = AMID_F64;
  }
  p.mid_in = cur;
  /* chain_mix :849-902 */
  if (user) {
    for (int ci = 0; ci < in.channels; ci++)
      for (int co = 0; co < out.channels; co++)
        m[ci * ms + co] = user[co * us + ci];           /* mix_matrix_from_g_value: the option is [out][in] */
  } else {
    default_mix_matrix (in.channels, in.position, in.unpositioned != 0, out.channels, out.position, m, ms);
  }
  /* gst_audio_channel_mixer_build_sparse_matrix (:1063-1122): with fewer than half of the coefficients above 1e-6 the mixer walks a
     list of those only - the others are not summed at all (which matters for float samples: inf * 0) */
  {
    int pairs = 0;
    for (int ci = 0; ci < in.channels; ci++)
      for (int co = 0; co < out.channels; co++)
        if (fabsf (m[ci * ms + co]) > 1e-6f)
          pairs++;
    p.sparse = (double) pairs / (double) (in.channels * out.channels) < 0.5 ? 1 : 0;
    for (int co = 0; co < out.channels; co++) {
      use[co] = 0;
      for (int ci = 0; ci < in.channels; ci++)
        if (!p.sparse || fabsf (m[ci * ms + co]) > 1e-6f)
          use[co] |= (uint64_t) 1 << ci;
    }
  }
  for (int ci = 0; ci < in.channels; ci++)
    for (int co = 0; co < out.channels; co++) {
      const float tmp = m[ci * ms + co] * (float) (1 << 10);    /* gst_audio_channel_mixer_setup_matrix_int */
      mi[ci * ms + co] = (int) tmp;
    }
  bool mix_passthrough = in.channels == out.channels && in_layout == out_layout;
  for (int i = 0; i < in.channels && mix_passthrough; i++)
    for (int j = 0; j < out.channels && mix_passthrough; j++)
      mix_passthrough = m[i * ms + j] == (i == j ? 1.0f : 0.0f);
  p.mix = mix_passthrough ? 0 : 1;
  /* chain_resample :904-943 */
  *resample = in.rate != out.rate || (flags & 2) != 0;
  /* chain_convert_out :945-966 */
  if (!fi.integer && fo.integer) {
    p.convert_out = 1;
    cur = AMID_S32;
  }
  p.mid_out = cur;
  /* chain_quantize :968-1022 */
  {
    const int in_depth = cur == AMID_S16 ? 16 : cur == AMID_F64 ? 64 : 32;
    const bool in_int = cur == AMID_S16 || cur == AMID_S32;
    int dither = cfg.dither_method, ns = cfg.noise_shaping;
    if ((unsigned) fo.depth > cfg.dither_threshold || (in_int && fo.depth >= in_depth)) {
      dither = GSTAMD_AUDIO_DITHER_NONE;
      ns = 0;
    } else if (ns > 1 && out.rate < 32000) {
      ns = 1;
    }
    if (fo.integer && fo.depth < 32 && cur == AMID_S32) {
      /* gst_audio_quantize_setup_noise_shaping :344-373 */
      static const double ns_simple[] = { -0.5, 1.0 };
      static const double ns_medium[] = { 0.6149, -1.590, 1.959, -2.165, 2.033 };
      static const double ns_high[] = { -0.340122, 0.876066, -1.72008, 2.61339, -3.31399, 3.27918, -2.92975, 2.08484 };
      const double *cf = ns == 2 ? ns_simple : ns == 3 ? ns_medium : ns_high;
      p.ns = ns;
      p.n_coeffs = ns == 2 ? 2 : ns == 3 ? 5 : ns == 4 ? 8 : 0;
      for (int i = 0; i < p.n_coeffs; i++)
        p.coeffs[i] = (int32_t) floor (cf[i] * 1024.0 + 0.5);
      if (ns < 0 || ns > 4 || dither < 0 || dither > 3) {
        *err = "unknown dither / noise shaping method";
        return GSTAMD_ERR_INVALID;
      }
      p.quant_shift = 32 - fo.depth;                    /* quantizer 1 << (32 - depth): count_power */
      p.dither = dither;
    }
  }
  /* "optimize" :1404-1453: same format, passthrough mixing, no resampler -> the bytes themselves */
  *passthrough = mix_passthrough && same_format && !*resample;
  /* the same, with formats that differ in byte order only: converter_endian, a byte swap of the samples as they are - no unpack, no
     quantize (so no dither), and floats are not looked at (denormals and NaN payloads pass) */
  if (mix_passthrough && !*resample && afmt_endian_pair (in.format, out.format)) {
    p.endian_swap = afmt_bytes (in.format);
    p.quant_shift = p.dither = p.ns = p.n_coeffs = 0;           /* this chain has no quantizer */
  }
  return GSTAMD_OK;
}

inline int aconv_make_plan_layouts (int flags, const GstAmdAudioInfo *in, int in_layout, const GstAmdAudioInfo *out, int out_layout,
    const GstAmdAudioConverterConfig &cfg, AConvPlan *plan, bool *resample, bool *passthrough, std::string *err)
{
  const AConvSide si = { in->format, in->rate, in->channels, in->layout, in->unpositioned, in->position };
  const AConvSide so = { out->format, out->rate, out->channels, out->layout, out->unpositioned, out->position };
  uint64_t use[GSTAMD_AUDIO_MAX_CHANNELS] = { 0 };
  memset (plan, 0, sizeof (*plan));
  const int r = aconv_plan_chain (flags, si, in_layout, so, out_layout, cfg, GSTAMD_AUDIO_MAX_CHANNELS, cfg.has_mix_matrix ? &cfg.mix_matrix[0][0] : nullptr,
      GSTAMD_AUDIO_MAX_CHANNELS, plan, &plan->m[0][0], &plan->mi[0][0], GSTAMD_AUDIO_MAX_CHANNELS, use, resample, passthrough, err);
  for (int co = 0; co < GSTAMD_AUDIO_MAX_CHANNELS; co++)
    plan->use[co] = (uint32_t) use[co];
  return r;
}

// gst_audio_converter_new with two interleaved infos
inline int aconv_make_plan (int flags, const GstAmdAudioInfo *in, const GstAmdAudioInfo *out, const GstAmdAudioConverterConfig &cfg, AConvPlan *plan,
    bool *resample, bool *passthrough, std::string *err)
{
  return aconv_make_plan_layouts (flags, in, 0, out, 0, cfg, plan, resample, passthrough, err);
}

// ---- the wide plan (1 .. 64 channels): the scalar fields of an AConvPlan - whose own m / mi / use stay zero -, and the
// matrices beside it as the mixing kernel reads them from device memory: [in][out] with row stride out_ch, a 64-bit use[out]
struct AConvWidePlan {
  AConvPlan s;
  std::vector<float> m;
  std::vector<int32_t> mi;
  std::vector<uint64_t> use;
};

// mix_matrix: NULL, or out->channels rows of in->channels floats
inline int aconv_make_plan_wide (int flags, const GstAmdAudioInfoWide *in, int in_layout, const GstAmdAudioInfoWide *out, int out_layout,
    const GstAmdAudioConverterConfig &cfg, const float *mix_matrix, AConvWidePlan *plan, bool *resample, bool *passthrough, std::string *err)
{
  if (cfg.has_mix_matrix) {
    *err = "config->has_mix_matrix is 0 here: the matrix is the mix_matrix argument of gstamd_audio_converter_new_wide";
    return GSTAMD_ERR_INVALID;
  }
  const AConvSide si = { in->format, in->rate, in->channels, in->layout, in->unpositioned, in->position };
  const AConvSide so = { out->format, out->rate, out->channels, out->layout, out->unpositioned, out->position };
  memset (&plan->s, 0, sizeof (plan->s));
  const bool counts = in->channels >= 1 && out->channels >= 1 && in->channels <= GSTAMD_AUDIO_MAX_CHANNELS_WIDE && out->channels <= GSTAMD_AUDIO_MAX_CHANNELS_WIDE;
  const size_t n = counts ? (size_t) in->channels * (size_t) out->channels : 1;
  plan->m.assign (n, 0.0f);
  plan->mi.assign (n, 0);
  plan->use.assign (GSTAMD_AUDIO_MAX_CHANNELS_WIDE, 0);
  static_assert (sizeof (int) == sizeof (int32_t), "mi");
  return aconv_plan_chain (flags, si, in_layout, so, out_layout, cfg, GSTAMD_AUDIO_MAX_CHANNELS_WIDE, mix_matrix, in->channels, &plan->s, plan->m.data (),
      (int *) plan->mi.data (), out->channels, plan->use.data (), resample, passthrough, err);
}

// ---- gstamd_audio_converter_samples_many: which streams of a call share a set of launches, the entries of a stream
// in the tables of the batched kernels, and the call itself as one walk over a backend - the device (audio_convert.hip, whose backend
// launches the kernels) or the host (tests/emu/emu_audio_many.cpp, whose backend loops over the grid of each launch).  What the two
// backends do not supply they cannot do differently.
//
// One stream of the call as the decision sees it; aconv_many_item makes it.  Streams with in_frames == 0 are skipped before the walk
// ("skipping empty buffer"): they do nothing, so they neither belong to a run nor end one.
struct AConvManyItem {
  const AConvPlan *plan;
  const void *id;               // the converter: the same one twice in a run would make its second buffer depend on its first
  bool ordinary;                // not wide, both layouts interleaved, not passthrough (the endian plan is read from the plan)
  bool resampler;               // a resampler sits between the two kernels
  bool has_input;               // in[i] != NULL
  size_t in_frames, out_frames;
  // A revision's tests, with their emulator sources (tests/emu), are also run against the next revision's library and headers.  Those of
  // the revision before the one walk (its emu_audio_many.cpp and emu_audio_many_layouts.cpp) fill this struct by position, the former
  // the seven members above alone: it leaves the rest zero and batches the ordinary converters only.  For them to build and to decide
  // as they did, `ordinary`, `layouts` and the order of the members stay for now; once no such source is run any more they can go,
  // and aconv_many_batchable then begins with !a.passthrough.
  bool layouts;                 // the caller has the batched kernels for non-interleaved and wide converters too: always, in aconv_many_item
  bool passthrough;
  bool wide;
  int in_layout, out_layout;
  const AConvWidePlan *wide_plan;       // of a wide converter: its matrices, which *plan does not hold
};

inline bool aconv_many_batchable (const AConvManyItem &a)
{
  return (a.ordinary || (a.layouts && !a.passthrough)) && !a.plan->endian_swap && a.has_input && a.in_frames > 0 && a.in_frames < ((size_t) 1 << 30) &&
      a.out_frames < ((size_t) 1 << 30);
}

// what two converters of a run share beside the bytes of their AConvPlan, which do not tell a non-interleaved from an interleaved mono
// output (q_stride is 1 in both) and hold no matrix of a wide converter
inline bool aconv_many_same_shape (const AConvManyItem &a, const AConvManyItem &b)
{
  if (a.in_layout != b.in_layout || a.out_layout != b.out_layout || a.wide != b.wide)
    return false;
  if (!a.wide)
    return true;
  const AConvWidePlan *x = a.wide_plan, *y = b.wide_plan;
  auto same = [](const auto &u, const auto &v) { return u.size () == v.size () && (u.empty () || memcmp (u.data (), v.data (), u.size () * sizeof (u[0])) == 0); };
  return x && y && same (x->m, y->m) && same (x->mi, y->mi) && same (x->use, y->use);
}

// The run that starts at it[0]: how many consecutive streams (at most GSTAMD_ACONV_MANY_MAX) one set of launches serves.  1: it[0] goes
// through the single-stream path by itself - because it does not qualify, or because its neighbour does not join it.
inline int aconv_many_run_length (const AConvManyItem *it, int n)
{
  if (n < 1)
    return 0;
  if (!aconv_many_batchable (it[0]))
    return 1;
  int run = 1;
  while (run < n && run < GSTAMD_ACONV_MANY_MAX) {
    const AConvManyItem &a = it[run];
    /* (an AConvPlan is zero-filled before it is made and has no padding: equal bytes are equal fields, matrices included) */
    if (!aconv_many_batchable (a) || a.resampler != it[0].resampler || memcmp (a.plan, it[0].plan, sizeof (AConvPlan)) != 0 || !aconv_many_same_shape (a, it[0]))
      break;
    bool dup = false;
    for (int k = 0; k < run; k++)
      dup = dup || it[k].id == a.id;
    if (dup)
      break;
    run++;
  }
  return run;
}

// ---- a stream's entries in the tables of the batched kernels; each returns the stream's lanes.  The splits are those of aconv_run's own
// launches: computed per stream, since every caller buffer has its own byte phase.
inline size_t aconv_many_pre_entry (const AConvPlan &p, const uint8_t *in, size_t in_frames, uint8_t *mid, AConvManyPre *e)
{
  const AConvSplit s = aconv_split (in, afmt_bytes (p.in_fmt), in_frames * (size_t) p.out_ch, aconv_pre_grouped (p));
  *e = { in, mid, aconv_split_pack (s) };
  return aconv_split_lanes (s);
}

inline size_t aconv_many_post_entry (const AConvPlan &p, const AConvDitherState &ds, const uint8_t *mid, uint8_t *out, size_t out_frames, int32_t *q, AConvManyPost *e)
{
  const AConvSplit s = aconv_split (out, afmt_bytes (p.out_fmt), out_frames * (size_t) p.out_ch, aconv_post_grouped (p));
  *e = { mid, out, q, aconv_split_pack (s), ds, 0 };
  return aconv_split_lanes (s);
}

inline bool aconv_plan_shapes (const AConvPlan &p) { return p.ns && p.quant_shift > 0; }

// aconv_run's own choice of its first kernel, from what a run shares
enum AConvManyFirst : int { ACONV_FIRST_PLAIN = 0, ACONV_FIRST_PLANES, ACONV_FIRST_MIX, ACONV_FIRST_WIDE };

inline int aconv_many_first (const AConvPlan &p, bool wide, int in_layout, int out_layout)
{
  if (wide && (in_layout || p.mix))
    return ACONV_FIRST_WIDE;
  if (in_layout)
    return ACONV_FIRST_PLANES;
  return out_layout && aconv_pre_grouped_mix (p) ? ACONV_FIRST_MIX : ACONV_FIRST_PLAIN;
}

// A side of `planes` planes at base, frames * bytes apart, for a launch whose rows are the planes themselves (rows_are_planes: each row
// takes the head of its own plane, on the device) or read all of them (one head where the planes reach a dword at the same frame,
// otherwise realign or a lane per frame): aconv_planes_heads for any channel count, in four bits.
inline AConvManySide aconv_many_side_entry (const uint8_t *base, size_t frames, int planes, int bytes, bool grouped, bool rows_are_planes)
{
  AConvManySide e = { (uint8_t *) base, (uint32_t) frames, 4u };
  if (!grouped)
    return e;
  if (rows_are_planes) {
    e.how = AConvPlanesEven::OWN;
    return e;
  }
  bool same = true;
  int h0 = 4;
  for (int c = 0; c < planes; c++) {
    const int h = aconv_head_at (base + (size_t) c * frames * (size_t) bytes, bytes, frames);
    h0 = c == 0 ? h : h0;
    same = same && h == h0;
  }
  e.how = same ? (uint32_t) h0 : 4u | (bytes < 4 && frames >= 12 ? 8u : 0u);
  return e;
}

// lanes of the longest row
inline size_t aconv_many_side_lanes (const AConvManySide &e, int bytes, int rows)
{
  const AConvPlanesEven pl = aconv_many_side (e, bytes);
  size_t m = 0;
  for (int y = 0; y < rows; y++) {
    const size_t l = aconv_split_lanes (aconv_plane_split_of (pl, y));
    m = l > m ? l : m;
  }
  return m;
}

inline size_t aconv_many_pre_planes_entry (const AConvPlan &p, const uint8_t *in, size_t in_frames, uint8_t *mid, AConvManyPrePlanes *e)
{
  const int b = afmt_bytes (p.in_fmt);
  *e = { aconv_many_side_entry (in, in_frames, p.in_ch, b, aconv_pre_grouped_planes (p), !p.mix), mid };
  return aconv_many_side_lanes (e->in, b, p.out_ch);
}

// interleaved frames into a converter whose layout changes: the split is of the FRAMES (aconv_pre_lane_mix)
inline size_t aconv_many_pre_mix_entry (const AConvPlan &p, const uint8_t *in, size_t in_frames, uint8_t *mid, AConvManyPre *e)
{
  const AConvSplit s = aconv_split (in, afmt_bytes (p.in_fmt) * p.in_ch, in_frames, true);
  *e = { in, mid, aconv_split_pack (s) };
  return aconv_split_lanes (s);
}

// the wide mixing kernel stages every run of samples by itself: no head.  Returns the stream's tiles.
inline size_t aconv_many_wide_entry (const uint8_t *in, size_t in_frames, uint8_t *mid, int tile, AConvManyPrePlanes *e)
{
  *e = { { (uint8_t *) in, (uint32_t) in_frames, 4u }, mid };
  return (in_frames + (size_t) tile - 1) / (size_t) tile;
}

inline size_t aconv_many_post_planes_entry (const AConvPlan &p, const AConvDitherState &ds, const uint8_t *mid, uint8_t *out, size_t out_frames, int32_t *q,
    AConvManyPostPlanes *e)
{
  const int b = afmt_bytes (p.out_fmt);
  *e = { mid, q, aconv_many_side_entry (out, out_frames, p.out_ch, b, aconv_post_grouped (p), true), ds, 0 };
  return aconv_many_side_lanes (e->out, b, p.out_ch);
}

// ---- the call ------------------------------------------------------------------------------------------------------------------------
// What the walk reads of a converter; a backend fills it from its own handle.
struct AConvManyConv {
  void *h;                      // the backend's handle, and the converter's identity; NULL: the call has no converter here
  const AConvPlan *plan;
  const AConvWidePlan *wide_plan;       // of a wide converter, else NULL
  bool wide, passthrough;
  int in_layout, out_layout;
  void *resampler;              // the backend's own, or NULL
  AConvDitherState *dither;
  const AConvJump *jump_host;
  int32_t *hist;                // where the shape launches find it
  const AConvJump *jump;        // where the post launches find the table: device memory on the device
  AConvWideMatrix matrix;       // the same of a wide converter's matrices
};

// a stream's buffers in a run, where the launches find them
struct AConvManyBuffers {
  uint8_t *mid_a, *mid_b;       // before / after the resampler (mid_b: NULL without one)
  int32_t *q;                   // the samples and, behind them, the dither words of a stream that shapes noise, else NULL
};

// a stream as aconv_many_run_length sees it: the one place that fills an item, for the library and the emulator alike
inline AConvManyItem aconv_many_item (const AConvManyConv &c, bool has_input, size_t in_frames, size_t out_frames)
{
  return { c.plan, c.h, !c.wide && !c.in_layout && !c.out_layout && !c.passthrough, c.resampler != nullptr, has_input, in_frames, out_frames, true, c.passthrough,
    c.wide, c.in_layout, c.out_layout, c.wide_plan };
}

// A backend B supplies
//   bool has_convs ()                                  the call's array of converters is not NULL
//   AConvManyConv conv (int i)                         converter i of the call
//   int fail (int code, const char *msg)               returns code
//   int single (c, in, in_frames, out, out_frames)     the single-stream call
//   int buffers (c, mid_a_bytes, mid_b_bytes, q_bytes, AConvManyBuffers *)     0 bytes: not needed, NULL
//   void pre / pre_planes / pre_mix (p, table, lanes, run), void wide_mix (p, matrix, table, in_layout, tile, tiles, run),
//   void post / post_planes (p, jump, table, lanes, run), void shape (p, table, run), void shape_planes (p, table)
//                                                      the batched launches, named after their kernels (k_aconv_<name>_many)
//   int resample_many (run, cs, buffers, in_frames, out_frames)
//   int launched ()                                    GSTAMD_OK unless a launch failed; the run needs its buffers no longer
//
// A run (aconv_many_run_length) of `run` >= 2 converters of one plan, layout pair and kind: aconv_run's stages, each as one launch over
// all of them.  record[3] counts the launches of the batched converter kernels.
template <typename B>
inline int aconv_many_run (B &be, int run, const AConvManyConv *cs, const uint8_t *const *in, const size_t *in_frames, uint8_t *const *out,
    const size_t *out_frames, int32_t *record)
{
  const AConvPlan &p = *cs[0].plan;
  const size_t mid_bytes_in = (size_t) amid_bytes (p.mid_in) * (size_t) p.out_ch;
  const bool shape = aconv_plan_shapes (p), resample = cs[0].resampler != nullptr;
  const int out_layout = cs[0].out_layout;
  AConvManyBuffers b[GSTAMD_ACONV_MANY_MAX];
  int r;
  /* every allocation before the first launch */
  for (int k = 0; k < run; k++)
    if ((r = be.buffers (cs[k], in_frames[k] * mid_bytes_in, resample ? (out_frames[k] ? out_frames[k] : 1) * mid_bytes_in : 0,
             shape && out_frames[k] ? out_frames[k] * (size_t) p.out_ch * 8 : 0, &b[k])) != GSTAMD_OK)
      return r;
  size_t lanes = 0;
  switch (aconv_many_first (p, cs[0].wide, cs[0].in_layout, out_layout)) {
    case ACONV_FIRST_WIDE: {
      AConvManyPrePlanesTable t;
      memset ((void *) &t, 0, sizeof (t));
      const int tile = aconv_wide_tile_frames (p.in_ch, p.out_ch);
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_wide_entry (in[k], in_frames[k], b[k].mid_a, tile, &t.s[k]);
        lanes = l > lanes ? l : lanes;          /* tiles, here */
      }
      be.wide_mix (p, cs[0].matrix, t, cs[0].in_layout, tile, lanes, run);      /* the matrix is the first converter's: a run shares it */
      break;
    }
    case ACONV_FIRST_PLANES: {
      AConvManyPrePlanesTable t;
      memset ((void *) &t, 0, sizeof (t));
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_pre_planes_entry (p, in[k], in_frames[k], b[k].mid_a, &t.s[k]);
        lanes = l > lanes ? l : lanes;
      }
      be.pre_planes (p, t, lanes, run);
      break;
    }
    case ACONV_FIRST_MIX: {
      AConvManyPreTable t;
      memset ((void *) &t, 0, sizeof (t));
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_pre_mix_entry (p, in[k], in_frames[k], b[k].mid_a, &t.s[k]);
        lanes = l > lanes ? l : lanes;
      }
      be.pre_mix (p, t, lanes, run);
      break;
    }
    default: {
      AConvManyPreTable t;
      memset ((void *) &t, 0, sizeof (t));
      for (int k = 0; k < run; k++) {
        const size_t l = aconv_many_pre_entry (p, in[k], in_frames[k], b[k].mid_a, &t.s[k]);
        lanes = l > lanes ? l : lanes;
      }
      be.pre (p, t, lanes, run);
      break;
    }
  }
  record[3]++;
  /* one launch where the filter qualifies, per stream where it does not: resample_many's own decision */
  if (resample && (r = be.resample_many (run, cs, b, in_frames, out_frames)) != GSTAMD_OK)
    return r;
  AConvManyShapeTable sh;
  memset ((void *) &sh, 0, sizeof (sh));
  lanes = 0;                                    /* stays 0 where every resampler of the run only took input into its history */
  if (out_layout) {
    AConvManyPostPlanesTable t;
    memset ((void *) &t, 0, sizeof (t));
    for (int k = 0; k < run; k++) {
      const size_t l = aconv_many_post_planes_entry (p, *cs[k].dither, resample ? b[k].mid_b : b[k].mid_a, out[k], out_frames[k], b[k].q, &t.s[k]);
      lanes = l > lanes ? l : lanes;
      sh.s[k] = { b[k].q, cs[k].hist, out[k], out_frames[k] };
    }
    if (lanes) {
      be.post_planes (p, cs[0].jump, t, lanes, run);
      record[3]++;
      if (shape) {
        be.shape_planes (p, sh);
        record[3]++;
      }
    }
  } else {
    AConvManyPostTable t;
    memset ((void *) &t, 0, sizeof (t));
    for (int k = 0; k < run; k++) {
      const size_t l = aconv_many_post_entry (p, *cs[k].dither, resample ? b[k].mid_b : b[k].mid_a, out[k], out_frames[k], b[k].q, &t.s[k]);
      lanes = l > lanes ? l : lanes;
      sh.s[k] = { b[k].q, cs[k].hist, out[k], out_frames[k] };
    }
    if (lanes) {
      be.post (p, cs[0].jump, t, lanes, run);
      record[3]++;
      if (shape) {
        be.shape (p, sh, run);
        record[3]++;
      }
    }
  }
  if ((r = be.launched ()) != GSTAMD_OK)
    return r;
  /* the generators move on by the draws of this call */
  for (int k = 0; k < run; k++)
    aconv_dither_advance (p, *cs[k].jump_host, cs[k].dither, out_frames[k] * (size_t) p.out_ch);
  return GSTAMD_OK;
}

// The whole call.  record: { batched runs, streams served by them, streams gone one by one, launches of the batched converter kernels }.
template <typename B>
inline int aconv_many_samples (B &be, int n, const void *const *in, const size_t *in_frames, void *const *out, const size_t *out_frames, int32_t *record)
{
  record[0] = record[1] = record[2] = record[3] = 0;
  if (n < 0 || (n > 0 && (!be.has_convs () || !in_frames || !out_frames)))
    return be.fail (GSTAMD_ERR_INVALID, "NULL argument array");
  /* everything that can refuse a stream, for all of them, before anything is launched: what gstamd_audio_converter_samples checks */
  std::vector<AConvManyConv> cv ((size_t) (n > 0 ? n : 0));       /* the view of every stream's converter, made once */
  for (int i = 0; i < n; i++) {
    const AConvManyConv &c = cv[(size_t) i] = be.conv (i);
    if (!c.h || (out_frames[i] && (!out || !out[i])))
      return be.fail (GSTAMD_ERR_INVALID, "NULL converter or output");
    if (in_frames[i] == 0)
      continue;
    if (!c.resampler && !(in && in[i]))
      return be.fail (GSTAMD_ERR_INVALID, "NULL input");
    if (!c.resampler && !c.passthrough && in_frames[i] != out_frames[i])
      return be.fail (GSTAMD_ERR_INVALID, "in_frames != out_frames without a resampler");
  }
  std::vector<AConvManyItem> items;
  std::vector<int> at;                          /* items[j] is stream at[j] of the call: the streams with in_frames == 0 are skipped here */
  items.reserve ((size_t) n);
  at.reserve ((size_t) n);
  for (int i = 0; i < n; i++) {
    if (in_frames[i] == 0)
      continue;
    items.push_back (aconv_many_item (cv[(size_t) i], in && in[i] != nullptr, in_frames[i], out_frames[i]));
    at.push_back (i);
  }
  const int live = (int) items.size ();
  for (int done = 0; done < live;) {
    const int run = aconv_many_run_length (&items[(size_t) done], live - done);
    int r;
    if (run < 2) {
      const int i = at[(size_t) done];
      r = be.single (cv[(size_t) i], in ? in[i] : nullptr, in_frames[i], out ? out[i] : nullptr, out_frames[i]);
      record[2]++;
    } else {
      AConvManyConv cs[GSTAMD_ACONV_MANY_MAX];
      const uint8_t *ip[GSTAMD_ACONV_MANY_MAX];
      uint8_t *op[GSTAMD_ACONV_MANY_MAX];
      size_t inf[GSTAMD_ACONV_MANY_MAX], outf[GSTAMD_ACONV_MANY_MAX];
      for (int k = 0; k < run; k++) {
        const int i = at[(size_t) (done + k)];
        cs[k] = cv[(size_t) i];
        ip[k] = (const uint8_t *) in[i];
        op[k] = out ? (uint8_t *) out[i] : nullptr;
        inf[k] = in_frames[i];
        outf[k] = out_frames[i];
      }
      r = aconv_many_run (be, run, cs, ip, inf, op, outf, record);
      record[0]++;
      record[1] += run;
    }
    if (r != GSTAMD_OK)
      return r;
    done += run;
  }
  return GSTAMD_OK;
}

}  // namespace gstamd
