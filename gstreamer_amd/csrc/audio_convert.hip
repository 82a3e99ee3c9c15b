// audio_convert.hip - GstAudioConverter on the device: the decision code of gst_audio_converter_new (audio-converter.c:1346-1470) restated
// on the host, two kernels around the resampler of audio_kernels.hip, and the C ABI of include/gstamd_audio.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/gstamd_audio.h"
#include "../../include/gstamd_video.h"
#include "audio_convert_device.h"
#include "audio_convert_plan.h"

using namespace gstamd;

extern "C" void gstamd_internal_set_error (const char *msg);

static int aconv_fail (int code, const std::string &msg)
{
  gstamd_internal_set_error (("audio converter: " + msg).c_str ());
  return code;
}

// ---- kernels: a lane per sample, or per four samples on aligned dwords (AConvSplit); one instance per container (AKind) ---------------
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_pre (AConvPlan p, const uint8_t *__restrict__ in, uint8_t *__restrict__ mid, AConvSplit s)
{
  const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= aconv_split_lanes (s))
    return;
  aconv_pre_lane<K> (p, in, mid, s, t);
}

template <int K>
__global__ __launch_bounds__ (256) void k_aconv_post (AConvPlan p, const AConvJump *__restrict__ jump, AConvDitherState ds, const uint8_t *__restrict__ mid,
    uint8_t *__restrict__ out, int32_t *__restrict__ qv, int32_t *__restrict__ qd, AConvSplit s)
{
  const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= aconv_split_lanes (s))
    return;
  aconv_post_lane<K> (p, *jump, ds, mid, out, qv, qd, s, t);
}

// noise shaping: the error recurrence of a channel is sequential in time, so one lane walks one channel's frames (the samples and
// dither words were prepared in parallel by k_aconv_post)
template <int K>
__global__ __launch_bounds__ (64) void k_aconv_shape (AConvPlan p, const int32_t *__restrict__ qv, const int32_t *__restrict__ qd, int32_t *__restrict__ hist,
    uint8_t *__restrict__ out, size_t frames)
{
  const int c = (int) threadIdx.x;
  if (c < p.out_ch)
    aconv_shape_channel<K> (p, qv, qd, hist, out, frames, c);
}

// the endian plan: the samples' bytes reversed (in may be out)
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_swap (const uint8_t *in, uint8_t *out, AConvSplit s)
{
  const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= aconv_split_lanes (s))
    return;
  aconv_swap_lane<K> (in, out, s, t);
}

// a non-interleaved side: blockIdx.y is the plane (for a mixing first kernel the output channel), the planes come by
// value in the kernel arguments.  Consecutive lanes are on consecutive addresses of a plane; the interleaved mid buffer is the strided side.
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_pre_planes (AConvPlan p, AConvPlanes src, uint8_t *__restrict__ mid)
{
  aconv_pre_lane_planes<K> (p, src, mid, (int) blockIdx.y, (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

// interleaved frames into a converter whose layout changes (so the mixer runs): blockIdx.y is the output channel, a lane takes four frames
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_pre_mix (AConvPlan p, const uint8_t *__restrict__ in, uint8_t *__restrict__ mid, AConvSplit s)
{
  aconv_pre_lane_mix<K> (p, in, mid, s, (int) blockIdx.y, (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

template <int K>
__global__ __launch_bounds__ (256) void k_aconv_post_planes (AConvPlan p, const AConvJump *__restrict__ jump, AConvDitherState ds, const uint8_t *__restrict__ mid,
    AConvPlanes dst, int32_t *__restrict__ qv, int32_t *__restrict__ qd)
{
  aconv_post_lane_planes<K> (p, *jump, ds, mid, dst, qv, qd, (int) blockIdx.y, (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

// noise shaping into planes: the reference's quantizer walks plane after plane with one channel's error history, so this is one
// recurrence over channels x frames samples - one lane
template <int K>
__global__ __launch_bounds__ (64) void k_aconv_shape_planes (AConvPlan p, const int32_t *__restrict__ qv, const int32_t *__restrict__ qd, int32_t *__restrict__ hist,
    AConvPlanes dst)
{
  if (threadIdx.x == 0)
    aconv_shape_planes<K> (p, qv, qd, hist, dst);
}

// ---- the wide converter (gstamd_audio_converter_new_wide) ----------------------------------------------------------------
// Its unmixed interleaved sides go through k_aconv_pre / k_aconv_post / k_aconv_shape above, which never look at a channel count beyond
// p.out_ch / p.q_stride.  The first kernel of every other case - a mix, a non-interleaved input - is this one: blockIdx.x is a tile of
// `tile` frames, staged once into LDS with the matrix and mixed from there (audio_convert_device.h).
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_wide_mix (AConvPlan p, AConvWideMatrix w, AConvPlanesWide src, int in_planar, uint8_t *__restrict__ mid, int tile)
{
  extern __shared__ __attribute__ ((aligned (16))) unsigned char aconv_wide_lds[];
  const size_t n0 = (size_t) blockIdx.x * (size_t) tile;
  if (n0 >= src.frames)
    return;
  const int nf = src.frames - n0 < (size_t) tile ? (int) (src.frames - n0) : tile;
  uint8_t *x = aconv_wide_lds, *mat = aconv_wide_lds + aconv_wide_x_bytes (p, tile);
  if (p.mix)
    aconv_wide_stage_matrix (p, w, mat, (int) threadIdx.x, 256);
  aconv_wide_stage_lane<K> (p, src, in_planar, n0, nf, x, (int) threadIdx.x, 256);
  __syncthreads ();
  aconv_wide_mix_lane (p, x, mat, w.use, mid, n0, nf, (int) threadIdx.x, 256);
}

template <int K>
__global__ __launch_bounds__ (256) void k_aconv_wide_post_planes (AConvPlan p, const AConvJump *__restrict__ jump, AConvDitherState ds, const uint8_t *__restrict__ mid,
    AConvPlanesWide dst, int32_t *__restrict__ qv, int32_t *__restrict__ qd)
{
  aconv_post_lane_planes_of<K> (p, *jump, ds, mid, dst, qv, qd, (int) blockIdx.y, (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

template <int K>
__global__ __launch_bounds__ (64) void k_aconv_wide_shape_planes (AConvPlan p, const int32_t *__restrict__ qv, const int32_t *__restrict__ qd, int32_t *__restrict__ hist,
    AConvPlanesWide dst)
{
  if (threadIdx.x == 0)
    aconv_shape_planes_of<K> (p, qv, qd, hist, dst);
}

// ---- many converters of one plan (gstamd_audio_converter_samples_many): blockIdx.y is the stream, blockIdx.x / the lane
// do what the stream's own k_aconv_pre / k_aconv_post launch would; the grid's x extent is the longest stream's, so the blocks past a
// shorter stream's lanes return at once.  The tables are indexed by blockIdx alone: scalar loads from the kernel arguments.
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_pre_many (AConvPlan p, AConvManyPreTable many)
{
  aconv_pre_many_lane<K> (p, many.s[blockIdx.y], (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

template <int K>
__global__ __launch_bounds__ (256) void k_aconv_post_many (AConvPlan p, const AConvJump *__restrict__ jump, AConvManyPostTable many)
{
  aconv_post_many_lane<K> (p, *jump, many.s[blockIdx.y], (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

// one 64-lane workgroup per stream, a lane per channel: the recurrences of all streams' channels walk at the same time
template <int K>
__global__ __launch_bounds__ (64) void k_aconv_shape_many (AConvPlan p, AConvManyShapeTable many)
{
  aconv_shape_many_lane<K> (p, many.s[blockIdx.x], (int) threadIdx.x);
}

// ---- the same for converters with a non-interleaved side and for wide ones.  A side of a stream is 16 bytes (one pointer,
// the planes frames * bytes apart), which the lane bodies of k_aconv_pre_planes / _post_planes / _shape_planes take as an AConvPlanesEven;
// since that struct has no pointer array it serves 64 channels as well as 8, and k_aconv_wide_post_planes / _shape_planes need no batched
// form of their own.  blockIdx.y: the row (an output channel), blockIdx.z: the stream.
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_pre_planes_many (AConvPlan p, AConvManyPrePlanesTable many)
{
  aconv_pre_planes_many_lane<K> (p, many.s[blockIdx.z], (int) blockIdx.y, (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

template <int K>
__global__ __launch_bounds__ (256) void k_aconv_pre_mix_many (AConvPlan p, AConvManyPreTable many)
{
  aconv_pre_mix_many_lane<K> (p, many.s[blockIdx.z], (int) blockIdx.y, (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

template <int K>
__global__ __launch_bounds__ (256) void k_aconv_post_planes_many (AConvPlan p, const AConvJump *__restrict__ jump, AConvManyPostPlanesTable many)
{
  aconv_post_planes_many_lane<K> (p, *jump, many.s[blockIdx.z], (int) blockIdx.y, (size_t) blockIdx.x * blockDim.x + threadIdx.x);
}

// ONE workgroup of 64 lanes, lane = stream: a stream's planes are one recurrence, so the 64 recurrences of a run walk side by side in one
// wave.  (The table is indexed by the lane here: vector loads from the kernel arguments; the entries past the run are zero.)
template <int K>
__global__ __launch_bounds__ (64) void k_aconv_shape_planes_many (AConvPlan p, AConvManyShapeTable many)
{
  aconv_shape_planes_many_lane<K> (p, many.s[threadIdx.x]);
}

// k_aconv_wide_mix with blockIdx.y = stream; a workgroup past its stream's last tile leaves as a whole before the barrier.  The matrix is
// the first converter's: aconv_many_run_length lets only converters of equal matrices share a run.
template <int K>
__global__ __launch_bounds__ (256) void k_aconv_wide_mix_many (AConvPlan p, AConvWideMatrix w, AConvManyPrePlanesTable many, int in_planar, int tile)
{
  extern __shared__ __attribute__ ((aligned (16))) unsigned char aconv_wide_lds[];
  const AConvManyPrePlanes &m = many.s[blockIdx.y];
  size_t n0;
  int nf;
  if (!aconv_wide_many_tile (m, (size_t) blockIdx.x, tile, &n0, &nf))
    return;
  uint8_t *x = aconv_wide_lds, *mat = aconv_wide_lds + aconv_wide_x_bytes (p, tile);
  if (p.mix)
    aconv_wide_stage_matrix (p, w, mat, (int) threadIdx.x, 256);
  aconv_wide_stage_lane<K> (p, aconv_many_side (m.in, akind_bytes (K)), in_planar, n0, nf, x, (int) threadIdx.x, 256);
  __syncthreads ();
  aconv_wide_mix_lane (p, x, mat, w.use, m.mid, n0, nf, (int) threadIdx.x, 256);
}

static unsigned aconv_blocks (const AConvSplit &s) { return (unsigned) ((aconv_split_lanes (s) + 255) / 256); }

struct GstAmdAudioConverter {
  GstAmdAudioInfo in, out;                              /* (not of a wide converter) */
  bool wide = false;                                    /* made by gstamd_audio_converter_new_wide: plan is wide_plan.s, the matrices are in device memory */
  AConvWidePlan wide_plan;
  AConvWideMatrix wide_dev = { nullptr, nullptr, nullptr };
  size_t hist_bytes = sizeof (int32_t) * 8 * GSTAMD_AUDIO_MAX_CHANNELS;
  GstAmdAudioConverterConfig cfg;
  int flags = 0;
  int in_layout = 0, out_layout = 0;                    /* GSTAMD_AUDIO_LAYOUT_* of the two sides */
  AConvPlan plan;
  bool passthrough = false;
  GstAmdAudioResampler *resampler = nullptr;
  AConvDitherState dither = { 0xc2d6038fu, 0u, 0 };     /* gst_audio_quantize_setup_dither */
  int32_t *hist = nullptr;                              /* [8][channels] noise shaping error history */
  uint8_t *q_v = nullptr, *q_d = nullptr;               /* S32 samples / dither words of a call with noise shaping */
  size_t q_v_size = 0, q_d_size = 0;
  AConvJump jump_host;
  AConvJump *jump_dev = nullptr;
  uint8_t *mid_a = nullptr, *mid_b = nullptr;           /* before / after the resampler */
  size_t mid_a_size = 0, mid_b_size = 0;
};

// what the two constructors share before the plan: how they refuse, and the config they run with
static GstAmdAudioConverter *aconv_new_fail (int *status, int code, const std::string &msg)
{
  aconv_fail (code, msg);
  if (status)
    *status = code;
  return nullptr;
}

static GstAmdAudioConverterConfig aconv_config_or_default (const GstAmdAudioConverterConfig *config)
{
  GstAmdAudioConverterConfig cfg;
  if (config)
    cfg = *config;
  else
    gstamd_audio_converter_config_init (&cfg);
  return cfg;
}

// what the two constructors share once the plan stands: the resampler, the jump table, the error history
static GstAmdAudioConverter *aconv_finish_new (GstAmdAudioConverter *c, bool resample, int in_rate, int out_rate, int *status)
{
  const GstAmdAudioConverterConfig &cfg = c->cfg;
  if (resample) {
    GstAmdAudioResamplerOptions ro;
    if (cfg.has_resampler_options)
      ro = cfg.resampler_options;
    else
      gstamd_audio_resampler_options_init (&ro);        /* the converter hands its (empty) config to the resampler: every key at its default */
    int st = 0;
    c->resampler = gstamd_audio_resampler_new (cfg.resampler_method, (c->flags & 2) ? 4 : 0, c->plan.mid_in, c->plan.out_ch, in_rate, out_rate, &ro, &st);
    if (!c->resampler) {
      gstamd_audio_converter_free (c);
      if (status)
        *status = st;
      return nullptr;
    }
  }
  auto fail = [&](const char *msg) -> GstAmdAudioConverter * {
    gstamd_audio_converter_free (c);
    const int code = aconv_fail (GSTAMD_ERR_HIP, msg);
    if (status)
      *status = code;
    return nullptr;
  };
  aconv_make_jump (&c->jump_host);
  if (hipMalloc ((void **) &c->jump_dev, sizeof (AConvJump)) != hipSuccess ||
      hipMemcpy (c->jump_dev, &c->jump_host, sizeof (AConvJump), hipMemcpyHostToDevice) != hipSuccess)
    return fail ("jump table upload");
  if (c->plan.ns) {
    /* (a null-stream memset returns before it has run and is not ordered against a non-blocking stream: wait for it - audio_kernels.hip ensure_hist) */
    if (hipMalloc ((void **) &c->hist, c->hist_bytes) != hipSuccess || hipMemset (c->hist, 0, c->hist_bytes) != hipSuccess || hipDeviceSynchronize () != hipSuccess)
      return fail ("error history");
  }
  if (status)
    *status = GSTAMD_OK;
  return c;
}

extern "C" {

void gstamd_audio_converter_config_init (GstAmdAudioConverterConfig *c)
{
  if (!c)
    return;
  memset (c, 0, sizeof (*c));
  /* DEFAULT_OPT_*, audio-converter.c:291-294 (the audioconvert element sets tpdf itself; the library's default is none) */
  c->dither_method = GSTAMD_AUDIO_DITHER_NONE;
  c->noise_shaping = 0;
  c->dither_threshold = 20;
  c->resampler_method = 3;                              /* GST_AUDIO_RESAMPLER_METHOD_BLACKMAN_NUTTALL */
}

GstAmdAudioConverter *gstamd_audio_converter_new (int flags, const GstAmdAudioInfo *in, const GstAmdAudioInfo *out, const GstAmdAudioConverterConfig *config,
    int *status)
{
  return gstamd_audio_converter_new_layouts (flags, in, GSTAMD_AUDIO_LAYOUT_INTERLEAVED, out, GSTAMD_AUDIO_LAYOUT_INTERLEAVED, config, status);
}

GstAmdAudioConverter *gstamd_audio_converter_new_layouts (int flags, const GstAmdAudioInfo *in, int in_layout, const GstAmdAudioInfo *out, int out_layout,
    const GstAmdAudioConverterConfig *config, int *status)
{
  if (!in || !out)
    return aconv_new_fail (status, GSTAMD_ERR_INVALID, "NULL info");
  const GstAmdAudioConverterConfig cfg = aconv_config_or_default (config);
  GstAmdAudioConverter *c = new GstAmdAudioConverter ();
  c->in = *in;
  c->out = *out;
  c->cfg = cfg;
  c->flags = flags;
  c->in_layout = in_layout;
  c->out_layout = out_layout;
  bool resample = false;
  std::string err;
  const int code = aconv_make_plan_layouts (flags, in, in_layout, out, out_layout, cfg, &c->plan, &resample, &c->passthrough, &err);
  if (code != GSTAMD_OK) {
    delete c;
    return aconv_new_fail (status, code, err);
  }
  return aconv_finish_new (c, resample, in->rate, out->rate, status);
}

GstAmdAudioConverter *gstamd_audio_converter_new_wide (int flags, const GstAmdAudioInfoWide *in, int in_layout, const GstAmdAudioInfoWide *out, int out_layout,
    const GstAmdAudioConverterConfig *config, const float *mix_matrix, int *status)
{
  if (!in || !out)
    return aconv_new_fail (status, GSTAMD_ERR_INVALID, "NULL info");
  const GstAmdAudioConverterConfig cfg = aconv_config_or_default (config);
  GstAmdAudioConverter *c = new GstAmdAudioConverter ();
  memset (&c->in, 0, sizeof (c->in));
  memset (&c->out, 0, sizeof (c->out));
  c->wide = true;
  c->cfg = cfg;
  c->flags = flags;
  c->in_layout = in_layout;
  c->out_layout = out_layout;
  c->hist_bytes = sizeof (int32_t) * 8 * GSTAMD_AUDIO_MAX_CHANNELS_WIDE;
  bool resample = false;
  std::string err;
  const int code = aconv_make_plan_wide (flags, in, in_layout, out, out_layout, cfg, mix_matrix, &c->wide_plan, &resample, &c->passthrough, &err);
  if (code != GSTAMD_OK) {
    delete c;
    return aconv_new_fail (status, code, err);
  }
  c->plan = c->wide_plan.s;
  /* the matrices: uploaded once, freed in _free */
  const size_t n = c->wide_plan.m.size ();
  float *m = nullptr;
  int32_t *mi = nullptr;
  uint64_t *use = nullptr;
  const bool up = hipMalloc ((void **) &m, 4 * n) == hipSuccess && hipMalloc ((void **) &mi, 4 * n) == hipSuccess &&
      hipMalloc ((void **) &use, 8 * GSTAMD_AUDIO_MAX_CHANNELS_WIDE) == hipSuccess &&
      hipMemcpy (m, c->wide_plan.m.data (), 4 * n, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy (mi, c->wide_plan.mi.data (), 4 * n, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy (use, c->wide_plan.use.data (), 8 * GSTAMD_AUDIO_MAX_CHANNELS_WIDE, hipMemcpyHostToDevice) == hipSuccess;
  c->wide_dev = { m, mi, use };
  if (!up) {
    gstamd_audio_converter_free (c);
    return aconv_new_fail (status, GSTAMD_ERR_HIP, "mix matrix upload");
  }
  return aconv_finish_new (c, resample, in->rate, out->rate, status);
}

void gstamd_audio_converter_free (GstAmdAudioConverter *c)
{
  if (!c)
    return;
  if (c->resampler)
    gstamd_audio_resampler_free (c->resampler);
  if (c->jump_dev)
    (void) hipFree (c->jump_dev);
  if (c->mid_a)
    (void) hipFree (c->mid_a);
  if (c->mid_b)
    (void) hipFree (c->mid_b);
  if (c->hist)
    (void) hipFree (c->hist);
  if (c->q_v)
    (void) hipFree (c->q_v);
  if (c->q_d)
    (void) hipFree (c->q_d);
  if (c->wide_dev.m)
    (void) hipFree ((void *) c->wide_dev.m);
  if (c->wide_dev.mi)
    (void) hipFree ((void *) c->wide_dev.mi);
  if (c->wide_dev.use)
    (void) hipFree ((void *) c->wide_dev.use);
  delete c;
}

void gstamd_audio_converter_reset (GstAmdAudioConverter *c)
{
  /* gst_audio_converter_reset (:1520-1530): the resampler and the quantizer, whose reset (audio-quantize.c:503-509) drops the error
     history and touches neither the random state nor last_random */
  if (c && c->resampler)
    gstamd_audio_resampler_reset (c->resampler);
  if (c && c->hist) {
    (void) hipDeviceSynchronize ();
    (void) hipMemset (c->hist, 0, c->hist_bytes);
    (void) hipDeviceSynchronize ();
  }
}

size_t gstamd_audio_converter_get_out_frames (GstAmdAudioConverter *c, size_t in_frames)
{
  return c && c->resampler ? gstamd_audio_resampler_get_out_frames (c->resampler, in_frames) : in_frames;
}

size_t gstamd_audio_converter_get_in_frames (GstAmdAudioConverter *c, size_t out_frames)
{
  return c && c->resampler ? gstamd_audio_resampler_get_in_frames (c->resampler, out_frames) : out_frames;
}

size_t gstamd_audio_converter_get_max_latency (GstAmdAudioConverter *c)
{
  return c && c->resampler ? gstamd_audio_resampler_get_max_latency (c->resampler) : 0;
}

int gstamd_audio_converter_is_passthrough (GstAmdAudioConverter *c) { return c && c->passthrough ? 1 : 0; }

int gstamd_audio_converter_get_mix_matrix (GstAmdAudioConverter *c, float *matrix, int max)
{
  if (!c || !matrix)
    return -1;
  int n = 0;
  for (int ci = 0; ci < c->plan.in_ch; ci++)
    for (int co = 0; co < c->plan.out_ch; co++, n++)
      if (n < max)
        matrix[n] = c->wide ? c->wide_plan.m[(size_t) ci * (size_t) c->plan.out_ch + (size_t) co] : c->plan.m[ci][co];
  return n;
}

static int ensure (uint8_t **buf, size_t *size, size_t need)
{
  if (*size >= need)
    return GSTAMD_OK;
  if (*buf)
    (void) hipFree (*buf);
  *buf = nullptr;
  *size = 0;
  if (hipMalloc ((void **) buf, need) != hipSuccess)
    return aconv_fail (GSTAMD_ERR_HIP, "hipMalloc(intermediate samples)");
  *size = need;
  return GSTAMD_OK;
}

// planes that follow one another without a gap are one run of samples
static bool planes_contiguous (uint8_t *const *pl, int n, size_t plane_bytes)
{
  for (int c = 1; c < n; c++)
    if (pl[c] != pl[c - 1] + plane_bytes)
      return false;
  return true;
}

static void swap_launch (int bytes, const uint8_t *in, uint8_t *out, size_t n, hipStream_t stream)
{
  const AConvSplit s = aconv_swap_split (in, out, bytes, n);
  if (aconv_split_lanes (s) == 0)
    return;
  switch (bytes) {
    case 2: k_aconv_swap<AK_2LE><<<dim3 (aconv_blocks (s)), dim3 (256), 0, stream>>> (in, out, s); break;
    case 3: k_aconv_swap<AK_3LE><<<dim3 (aconv_blocks (s)), dim3 (256), 0, stream>>> (in, out, s); break;
    case 4: k_aconv_swap<AK_4LE><<<dim3 (aconv_blocks (s)), dim3 (256), 0, stream>>> (in, out, s); break;
    default: k_aconv_swap<AK_8LE><<<dim3 (aconv_blocks (s)), dim3 (256), 0, stream>>> (in, out, s); break;
  }
}

// in[] / out[]: one pointer for an interleaved side, `channels` pointers for a non-interleaved one; in == NULL: silence
static int aconv_run (GstAmdAudioConverter *c, uint8_t *const *in, size_t in_frames, uint8_t *const *out, size_t out_frames, hipStream_t stream)
{
  const AConvPlan &p = c->plan;
  const size_t in_b = (size_t) afmt_bytes (p.in_fmt), out_b = (size_t) afmt_bytes (p.out_fmt);
  if (c->passthrough || p.endian_swap) {                /* equal layouts and channel counts: block by block */
    if (!in)
      return aconv_fail (GSTAMD_ERR_INVALID, "NULL input");
    if (!c->passthrough && in_frames != out_frames)
      return aconv_fail (GSTAMD_ERR_INVALID, "in_frames != out_frames without a resampler");
    int blocks = c->out_layout ? p.out_ch : 1;
    size_t n = out_frames * (size_t) (c->out_layout ? 1 : p.out_ch);   /* samples of a block */
    if (blocks > 1 && planes_contiguous (in, blocks, n * in_b) && planes_contiguous (out, blocks, n * out_b)) {
      n *= (size_t) blocks;
      blocks = 1;
    }
    for (int b = 0; b < blocks; b++) {
      if (c->passthrough) {
        if (in[b] != out[b] && n && hipMemcpyAsync (out[b], in[b], n * out_b, hipMemcpyDeviceToDevice, stream) != hipSuccess)
          return aconv_fail (GSTAMD_ERR_HIP, "copy");
      } else {
        swap_launch (p.endian_swap, in[b], out[b], n, stream);
      }
    }
    if (!c->passthrough && hipGetLastError () != hipSuccess)
      return aconv_fail (GSTAMD_ERR_HIP, "kernel launch");
    return GSTAMD_OK;
  }
  if (!c->resampler && in_frames != out_frames)
    return aconv_fail (GSTAMD_ERR_INVALID, "in_frames != out_frames without a resampler");
  const size_t mid_bytes_in = (size_t) amid_bytes (p.mid_in) * (size_t) p.out_ch;
  int r;
  const uint8_t *after = nullptr;
  if (in) {
    if ((r = ensure (&c->mid_a, &c->mid_a_size, (in_frames ? in_frames : 1) * mid_bytes_in)) != GSTAMD_OK)
      return r;
    if (c->wide && (c->in_layout || p.mix)) {
      AConvPlanesWide src;
      memset (&src, 0, sizeof (src));
      for (int ci = 0; ci < (c->in_layout ? p.in_ch : 1); ci++)
        src.p[ci] = in[ci];
      src.frames = in_frames;
      const int tile = aconv_wide_tile_frames (p.in_ch, p.out_ch);
      const size_t lds = aconv_wide_lds_bytes (p, tile);        /* at most 256 * 9 * 8 + 4 * 64 bytes of samples, 16 KB of matrix */
      if (in_frames) {
#define PRE(K) k_aconv_wide_mix<K><<<dim3 ((unsigned) ((in_frames + (size_t) tile - 1) / (size_t) tile)), dim3 (256), lds, stream>>> (p, c->wide_dev, src, c->in_layout, \
    c->mid_a, tile)
        GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
      }
    } else if (c->in_layout) {
      AConvPlanes src;
      memset (&src, 0, sizeof (src));
      for (int ci = 0; ci < p.in_ch; ci++)
        src.p[ci] = in[ci];
      src.frames = in_frames;
      aconv_planes_heads (&src, p.in_ch, p.out_ch, (int) in_b, aconv_pre_grouped_planes (p), !p.mix);
      const size_t lanes = aconv_planes_lanes (src, p.out_ch);
      if (lanes) {
#define PRE(K) k_aconv_pre_planes<K><<<dim3 ((unsigned) ((lanes + 255) / 256), (unsigned) p.out_ch), dim3 (256), 0, stream>>> (p, src, c->mid_a)
        GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
      }
    } else if (in_frames && c->out_layout && aconv_pre_grouped_mix (p)) {
      const AConvSplit s = aconv_split (in[0], (int) in_b * p.in_ch, in_frames, true);          /* of the frames */
#define PRE(K) k_aconv_pre_mix<K><<<dim3 (aconv_blocks (s), (unsigned) p.out_ch), dim3 (256), 0, stream>>> (p, in[0], c->mid_a, s)
      GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
    } else if (in_frames) {
      const AConvSplit s = aconv_split (in[0], (int) in_b, in_frames * (size_t) p.out_ch, aconv_pre_grouped (p));
#define PRE(K) k_aconv_pre<K><<<dim3 (aconv_blocks (s)), dim3 (256), 0, stream>>> (p, in[0], c->mid_a, s)
      GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
    }
    after = c->mid_a;
  } else if (!c->resampler) {
    return aconv_fail (GSTAMD_ERR_INVALID, "NULL input");
  }
  if (c->resampler) {
    if ((r = ensure (&c->mid_b, &c->mid_b_size, (out_frames ? out_frames : 1) * mid_bytes_in)) != GSTAMD_OK)
      return r;
    r = gstamd_audio_resampler_resample (c->resampler, in ? c->mid_a : nullptr, in_frames, c->mid_b, out_frames, stream);
    if (r != GSTAMD_OK)
      return r;
    after = c->mid_b;
  }
  const size_t samples = out_frames * (size_t) p.out_ch;
  if (samples == 0)                             /* the resampler only took input into its history */
    return GSTAMD_OK;
  const bool shape = p.ns && p.quant_shift > 0;
  if (shape) {
    if ((r = ensure (&c->q_v, &c->q_v_size, samples * 4)) != GSTAMD_OK || (r = ensure (&c->q_d, &c->q_d_size, samples * 4)) != GSTAMD_OK)
      return r;
  }
  if (c->out_layout && c->wide) {
    AConvPlanesWide dst;
    memset (&dst, 0, sizeof (dst));
    for (int co = 0; co < p.out_ch; co++)
      dst.p[co] = out[co];
    dst.frames = out_frames;
    aconv_planes_heads_wide (&dst, p.out_ch, (int) out_b, aconv_post_grouped (p));
    const size_t lanes = aconv_planes_lanes_wide (dst, p.out_ch);
#define POST(K) k_aconv_wide_post_planes<K><<<dim3 ((unsigned) ((lanes + 255) / 256), (unsigned) p.out_ch), dim3 (256), 0, stream>>> (p, c->jump_dev, c->dither, after, dst, \
    (int32_t *) c->q_v, (int32_t *) c->q_d)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
    if (shape) {
#define SHAPE(K) k_aconv_wide_shape_planes<K><<<dim3 (1), dim3 (64), 0, stream>>> (p, (const int32_t *) c->q_v, (const int32_t *) c->q_d, c->hist, dst)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
    }
  } else if (c->out_layout) {
    AConvPlanes dst;
    memset (&dst, 0, sizeof (dst));
    for (int co = 0; co < p.out_ch; co++)
      dst.p[co] = out[co];
    dst.frames = out_frames;
    aconv_planes_heads (&dst, p.out_ch, p.out_ch, (int) out_b, aconv_post_grouped (p), true);
    const size_t lanes = aconv_planes_lanes (dst, p.out_ch);
#define POST(K) k_aconv_post_planes<K><<<dim3 ((unsigned) ((lanes + 255) / 256), (unsigned) p.out_ch), dim3 (256), 0, stream>>> (p, c->jump_dev, c->dither, after, dst, \
    (int32_t *) c->q_v, (int32_t *) c->q_d)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
    if (shape) {
#define SHAPE(K) k_aconv_shape_planes<K><<<dim3 (1), dim3 (64), 0, stream>>> (p, (const int32_t *) c->q_v, (const int32_t *) c->q_d, c->hist, dst)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
    }
  } else {
    const AConvSplit s = aconv_split (out[0], (int) out_b, samples, aconv_post_grouped (p));
#define POST(K) k_aconv_post<K><<<dim3 (aconv_blocks (s)), dim3 (256), 0, stream>>> (p, c->jump_dev, c->dither, after, out[0], (int32_t *) c->q_v, \
    (int32_t *) c->q_d, s)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
    if (shape) {
#define SHAPE(K) k_aconv_shape<K><<<dim3 (1), dim3 (64), 0, stream>>> (p, (const int32_t *) c->q_v, (const int32_t *) c->q_d, c->hist, out[0], out_frames)
      GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
    }
  }
  if (hipGetLastError () != hipSuccess)
    return aconv_fail (GSTAMD_ERR_HIP, "kernel launch");
  /* the generator moves on by the draws of this call (setup_dither_buf draws for every sample of the block) */
  aconv_dither_advance (p, c->jump_host, &c->dither, samples);
  return GSTAMD_OK;
}

int gstamd_audio_converter_samples_planes (GstAmdAudioConverter *c, int flags, const void *const in[], size_t in_frames, void *const out[], size_t out_frames,
    void *stream)
{
  (void) flags;
  if (!c || (!out && out_frames))
    return aconv_fail (GSTAMD_ERR_INVALID, "NULL converter or output");
  if (in_frames == 0)                           /* gst_audio_converter_samples :1618-1621: "skipping empty buffer" */
    return GSTAMD_OK;
  uint8_t *ip[GSTAMD_AUDIO_MAX_CHANNELS_WIDE] = { nullptr }, *op[GSTAMD_AUDIO_MAX_CHANNELS_WIDE] = { nullptr };
  for (int k = 0; in && k < (c->in_layout ? c->plan.in_ch : 1); k++)
    if (!(ip[k] = (uint8_t *) in[k]))
      return aconv_fail (GSTAMD_ERR_INVALID, "NULL input plane");
  for (int k = 0; out_frames && k < (c->out_layout ? c->plan.out_ch : 1); k++)
    if (!(op[k] = (uint8_t *) out[k]))
      return aconv_fail (GSTAMD_ERR_INVALID, "NULL output plane");
  return aconv_run (c, in ? ip : nullptr, in_frames, op, out_frames, (hipStream_t) stream);
}

int gstamd_audio_converter_samples (GstAmdAudioConverter *c, int flags, const void *in, size_t in_frames, void *out, size_t out_frames, void *stream)
{
  (void) flags;
  if (!c || (!out && out_frames))
    return aconv_fail (GSTAMD_ERR_INVALID, "NULL converter or output");
  if (in_frames == 0)
    return GSTAMD_OK;
  /* a non-interleaved side as gstamd_audio_resampler_resample takes it: the channels one after the other, in_frames (out_frames) samples apart */
  uint8_t *ip[GSTAMD_AUDIO_MAX_CHANNELS_WIDE] = { nullptr }, *op[GSTAMD_AUDIO_MAX_CHANNELS_WIDE] = { nullptr };
  const size_t in_plane = in_frames * (size_t) afmt_bytes (c->plan.in_fmt), out_plane = out_frames * (size_t) afmt_bytes (c->plan.out_fmt);
  for (int k = 0; in && k < (c->in_layout ? c->plan.in_ch : 1); k++)
    ip[k] = (uint8_t *) in + (size_t) k * in_plane;
  for (int k = 0; k < (c->out_layout ? c->plan.out_ch : 1); k++)
    op[k] = (uint8_t *) out + (size_t) k * out_plane;
  return aconv_run (c, in ? ip : nullptr, in_frames, op, out_frames, (hipStream_t) stream);
}

/* ---- gstamd_audio_converter_samples_many: aconv_many_samples of audio_convert_plan.h over this backend ------------------ */
/* the calling thread's last call: batched runs, streams served by them, streams gone one by one, launches of the batched converter kernels */
static thread_local int32_t aconv_many_debug[4] = { 0, 0, 0, 0 };

namespace {
struct AConvManyDevice {
  GstAmdAudioConverter *const *convs;
  int flags;
  hipStream_t stream;

  bool has_convs () const { return convs != nullptr; }

  AConvManyConv conv (int i) const
  {
    GstAmdAudioConverter *c = convs[i];
    if (!c)
      return {};
    return { c, &c->plan, c->wide ? &c->wide_plan : nullptr, c->wide, c->passthrough, c->in_layout, c->out_layout, c->resampler, &c->dither, &c->jump_host, c->hist,
      c->jump_dev, c->wide_dev };
  }

  int fail (int code, const char *msg) { return aconv_fail (code, msg); }

  int single (const AConvManyConv &c, const void *in, size_t in_frames, void *out, size_t out_frames)
  {
    return gstamd_audio_converter_samples ((GstAmdAudioConverter *) c.h, flags, in, in_frames, out, out_frames, stream);
  }

  int buffers (const AConvManyConv &cv, size_t mid_a_bytes, size_t mid_b_bytes, size_t q_bytes, AConvManyBuffers *b)
  {
    GstAmdAudioConverter *c = (GstAmdAudioConverter *) cv.h;
    int r;
    if ((r = ensure (&c->mid_a, &c->mid_a_size, mid_a_bytes)) != GSTAMD_OK)
      return r;
    if (mid_b_bytes && (r = ensure (&c->mid_b, &c->mid_b_size, mid_b_bytes)) != GSTAMD_OK)
      return r;
    /* the samples and, behind them, the dither words (q_d stays the single-stream path's) */
    if (q_bytes && (r = ensure (&c->q_v, &c->q_v_size, q_bytes)) != GSTAMD_OK)
      return r;
    *b = { c->mid_a, mid_b_bytes ? c->mid_b : nullptr, q_bytes ? (int32_t *) c->q_v : nullptr };
    return GSTAMD_OK;
  }

  static unsigned blocks (size_t lanes) { return (unsigned) ((lanes + 255) / 256); }

  void wide_mix (const AConvPlan &p, const AConvWideMatrix &w, const AConvManyPrePlanesTable &t, int in_layout, int tile, size_t tiles, int run)
  {
    const size_t lds = aconv_wide_lds_bytes (p, tile);          /* of the plan: one value for the launch */
#define PRE(K) k_aconv_wide_mix_many<K><<<dim3 ((unsigned) tiles, (unsigned) run), dim3 (256), lds, stream>>> (p, w, t, in_layout, tile)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }

  void pre_planes (const AConvPlan &p, const AConvManyPrePlanesTable &t, size_t lanes, int run)
  {
#define PRE(K) k_aconv_pre_planes_many<K><<<dim3 (blocks (lanes), (unsigned) p.out_ch, (unsigned) run), dim3 (256), 0, stream>>> (p, t)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }

  void pre_mix (const AConvPlan &p, const AConvManyPreTable &t, size_t lanes, int run)
  {
#define PRE(K) k_aconv_pre_mix_many<K><<<dim3 (blocks (lanes), (unsigned) p.out_ch, (unsigned) run), dim3 (256), 0, stream>>> (p, t)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }

  void pre (const AConvPlan &p, const AConvManyPreTable &t, size_t lanes, int run)
  {
#define PRE(K) k_aconv_pre_many<K><<<dim3 (blocks (lanes), (unsigned) run), dim3 (256), 0, stream>>> (p, t)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }

  void post_planes (const AConvPlan &p, const AConvJump *jump, const AConvManyPostPlanesTable &t, size_t lanes, int run)
  {
#define POST(K) k_aconv_post_planes_many<K><<<dim3 (blocks (lanes), (unsigned) p.out_ch, (unsigned) run), dim3 (256), 0, stream>>> (p, jump, t)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
  }

  void shape_planes (const AConvPlan &p, const AConvManyShapeTable &sh)
  {
#define SHAPE(K) k_aconv_shape_planes_many<K><<<dim3 (1), dim3 (64), 0, stream>>> (p, sh)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
  }

  void post (const AConvPlan &p, const AConvJump *jump, const AConvManyPostTable &t, size_t lanes, int run)
  {
#define POST(K) k_aconv_post_many<K><<<dim3 (blocks (lanes), (unsigned) run), dim3 (256), 0, stream>>> (p, jump, t)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
  }

  void shape (const AConvPlan &p, const AConvManyShapeTable &sh, int run)
  {
#define SHAPE(K) k_aconv_shape_many<K><<<dim3 ((unsigned) run), dim3 (64), 0, stream>>> (p, sh)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
  }

  int resample_many (int run, const AConvManyConv *cs, const AConvManyBuffers *b, const size_t *in_frames, const size_t *out_frames)
  {
    GstAmdAudioResampler *rs[GSTAMD_ACONV_MANY_MAX];
    const void *ri[GSTAMD_ACONV_MANY_MAX];
    void *ro[GSTAMD_ACONV_MANY_MAX];
    for (int k = 0; k < run; k++) {
      rs[k] = (GstAmdAudioResampler *) cs[k].resampler;
      ri[k] = b[k].mid_a;
      ro[k] = b[k].mid_b;
    }
    return gstamd_audio_resampler_resample_many (run, rs, ri, in_frames, ro, out_frames, stream);
  }

  int launched () { return hipGetLastError () != hipSuccess ? aconv_fail (GSTAMD_ERR_HIP, "kernel launch") : GSTAMD_OK; }
};
}  // namespace

int gstamd_audio_converter_samples_many (int n, GstAmdAudioConverter *const *converters, int flags, const void *const *in, const size_t *in_frames,
    void *const *out, const size_t *out_frames, void *stream)
{
  AConvManyDevice be = { converters, flags, (hipStream_t) stream };
  return aconv_many_samples (be, n, in, in_frames, out, out_frames, aconv_many_debug);
}

int gstamd_audio_converter_debug_many (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = aconv_many_debug[i];
  return 4;
}

}  // extern "C"
