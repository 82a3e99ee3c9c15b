/* gstamd_audio.h - C ABI of the MI355X-native GstAudioResampler replacement (polyphase FIR).
 *
 * Drop-in boundary for the audio half of the hot path.  Reference interface being
 * replaced (subprojects/gst-plugins-base/gst-libs/gst/audio/audio-resampler.h):
 *
 *   gstamd_audio_resampler_options_set_quality <- gst_audio_resampler_options_set_quality  :218
 *   gstamd_audio_resampler_new                 <- gst_audio_resampler_new                  :224
 *   gstamd_audio_resampler_free / _reset       <- gst_audio_resampler_free / _reset        :231, :234
 *   gstamd_audio_resampler_get_out_frames      <- gst_audio_resampler_get_out_frames       :242
 *   gstamd_audio_resampler_get_in_frames       <- gst_audio_resampler_get_in_frames        :246
 *   gstamd_audio_resampler_get_max_latency     <- gst_audio_resampler_get_max_latency      :250
 *   gstamd_audio_resampler_resample(_planes)   <- gst_audio_resampler_resample             :253
 *
 * Sample buffers are DEVICE pointers (interleaved frames); the FIR runs as HIP kernels on `stream`
 * (hipStream_t as void*, NULL = default stream) and the call returns without synchronising.  All
 * bookkeeping (history length, sample index/phase, skip) is host state that follows the reference
 * function for function, so get_out_frames() etc. give the reference's numbers.  The taps tables are
 * computed on the host with the reference's double-precision recipe and uploaded once.
 * Float summation order is the reference's C order (4 interleaved partial sums, ((r0+r1)+r2)+r3,
 * audio-resampler.c:693-707), without FMA contraction: results are bit-identical to the C path.
 */
#ifndef GSTAMD_AUDIO_H
#define GSTAMD_AUDIO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* GstAudioResamplerMethod (audio-resampler.h:181-187) */
enum {
  GSTAMD_AUDIO_RESAMPLER_METHOD_NEAREST = 0, GSTAMD_AUDIO_RESAMPLER_METHOD_LINEAR = 1,
  GSTAMD_AUDIO_RESAMPLER_METHOD_CUBIC = 2, GSTAMD_AUDIO_RESAMPLER_METHOD_BLACKMAN_NUTTALL = 3,
  GSTAMD_AUDIO_RESAMPLER_METHOD_KAISER = 4
};
/* GstAudioResamplerFilterMode / FilterInterpolation (audio-resampler.h:103-107, 137-141) */
enum { GSTAMD_AUDIO_FILTER_MODE_INTERPOLATED = 0, GSTAMD_AUDIO_FILTER_MODE_FULL = 1, GSTAMD_AUDIO_FILTER_MODE_AUTO = 2 };
enum { GSTAMD_AUDIO_FILTER_INTERPOLATION_NONE = 0, GSTAMD_AUDIO_FILTER_INTERPOLATION_LINEAR = 1,
  GSTAMD_AUDIO_FILTER_INTERPOLATION_CUBIC = 2 };
/* gstamd_audio_resampler_new's `format` is a GstAudioFormat like gst_audio_resampler_new's (audio-resampler.h:218) - GSTAMD_AFMT_S16LE,
 * _S32LE, _F32LE, _F64LE below, whose values are GstAudioFormat's: a binding passes GST_AUDIO_INFO_FORMAT through.  The private
 * values 0 .. 3 of the first two releases stay understood (they collide with no GstAudioFormat the resampler accepts). */
enum { GSTAMD_AUDIO_FORMAT_S16 = 0, GSTAMD_AUDIO_FORMAT_S32 = 1, GSTAMD_AUDIO_FORMAT_F32 = 2, GSTAMD_AUDIO_FORMAT_F64 = 3 };

/* Mirror of the GstAudioResampler.* option keys (audio-resampler.h:42-165).  A field left at its
 * "unset" value (NaN for doubles, -1 for ints) means the key is absent from the options structure. */
typedef struct GstAmdAudioResamplerOptions {
  double cutoff;                 /* GstAudioResampler.cutoff */
  double stop_attenuation;       /* GstAudioResampler.stop-attenutation */
  double transition_bandwidth;   /* GstAudioResampler.transition-bandwidth */
  double cubic_b, cubic_c;       /* GstAudioResampler.cubic-b / cubic-c */
  double max_phase_error;        /* GstAudioResampler.max-phase-error */
  int32_t n_taps;                /* GstAudioResampler.n-taps */
  int32_t filter_mode;           /* GstAudioResampler.filter-mode */
  int32_t filter_mode_threshold; /* GstAudioResampler.filter-mode-threshold */
  int32_t filter_interpolation;  /* GstAudioResampler.filter-interpolation */
  int32_t filter_oversample;     /* GstAudioResampler.filter-oversample */
  int32_t reserved[7];
} GstAmdAudioResamplerOptions;

typedef struct GstAmdAudioResampler GstAmdAudioResampler;

/* all keys unset (an empty options structure) */
void gstamd_audio_resampler_options_init (GstAmdAudioResamplerOptions *options);
void gstamd_audio_resampler_options_set_quality (int method, unsigned quality, int in_rate, int out_rate,
    GstAmdAudioResamplerOptions *options);

/* options == NULL: Kaiser quality 4 like the reference (audio-resampler.c:1414-1419).  flags: GstAudioResamplerFlags
 * (audio-resampler.h:177-182) - 1 non-interleaved input, 2 non-interleaved output, 4 variable rate.  Returns NULL and sets *status (GSTAMD_ERR_* of gstamd_video.h) on failure.  Both filter
 * modes are implemented: FULL (one row of taps per phase) and INTERPOLATED (the taps of every output sample are blended
 * on the device from the oversampled table, linear or cubic, audio-resampler.c:567-757). */
GstAmdAudioResampler *gstamd_audio_resampler_new (int method, int flags, int format, int channels, int in_rate,
    int out_rate, const GstAmdAudioResamplerOptions *options, int *status);
void gstamd_audio_resampler_free (GstAmdAudioResampler *resampler);
void gstamd_audio_resampler_reset (GstAmdAudioResampler *resampler);
/* gst_audio_resampler_update (audio-resampler.h:231, audio-resampler.c:1503-1614): new rates (<= 0: unchanged) and / or new
 * options on a running stream; the phase is rescaled, and when the tap count changes the history moves by half the difference.
 * options == NULL keeps the previous filter design, as the reference does.  Returns GSTAMD_OK (the reference's TRUE) or an
 * error with the resampler left as it was. */
int gstamd_audio_resampler_update (GstAmdAudioResampler *resampler, int in_rate, int out_rate,
    const GstAmdAudioResamplerOptions *options);
/* Where the reference's own result is not a function of the stream: gst_audio_resampler_update with options that ENLARGE the filter by more than
 * twice the history it holds leaves the head of the new history as it finds it in its sample buffer - input of earlier calls past the valid
 * samples ("FIXME, probably do something better like mirror or fill with zeroes", audio-resampler.c:1587-1590).  This library fills those
 * frames with silence and says so here: a text while such frames are inside the filter window, "" otherwise (and always for streams that
 * never enlarge their filter that far).  Same contract as gstamd_video_converter_divergence. */
const char *gstamd_audio_resampler_divergence (GstAmdAudioResampler *resampler);
size_t gstamd_audio_resampler_get_out_frames (GstAmdAudioResampler *resampler, size_t in_frames);
size_t gstamd_audio_resampler_get_in_frames (GstAmdAudioResampler *resampler, size_t out_frames);
size_t gstamd_audio_resampler_get_max_latency (GstAmdAudioResampler *resampler);

/* in: device pointer to in_frames interleaved frames, or NULL for silence (drain); out: device pointer
 * with room for out_frames frames.  A non-interleaved side holds its channels one after the other, in_frames
 * (out_frames) samples apart. */
int gstamd_audio_resampler_resample (GstAmdAudioResampler *resampler, const void *in, size_t in_frames, void *out,
    size_t out_frames, void *stream);

/* gst_audio_resampler_resample's own argument shape (audio-resampler.h:253): in[] / out[] hold ONE pointer for an
 * interleaved side and `channels` pointers for a non-interleaved one (equally spaced planes in ascending order; anything
 * else is GSTAMD_ERR_UNSUPPORTED); in == NULL feeds silence. */
int gstamd_audio_resampler_resample_planes (GstAmdAudioResampler *resampler, const void *const in[], size_t in_frames,
    void *const out[], size_t out_frames, void *stream);

/* `n` independent resamplers, one buffer each (in[i] / out[i] interleaved, or non-interleaved planes following each other as in _resample),
 * in ONE kernel launch where they share a filter - resamplers made with the same arguments, in full or in interpolated filter mode (equal
 * filter mode, interpolation, oversampling and taps table), whose plan fits the 64 KB of LDS the staged kernels work in; up to 64 per
 * launch, longer or mixed sets run as several launches / one by one.  Outputs and resampler states are exactly those of n _resample calls.  For what
 * carries many streams at once: the channels of a non-interleaved capture, the inputs of a mixer, a buffer list.  No reference counterpart:
 * gst_audio_resampler_resample (audio-resampler.h:253) takes one stream and the reference has no cross-stream batching. */
int gstamd_audio_resampler_resample_many (int n, GstAmdAudioResampler *const *resamplers, const void *const *in, const size_t *in_frames,
    void *const *out, const size_t *out_frames, void *stream);

/* introspection for tests: n_taps, n_phases (reduced out_rate), reduced in_rate, oversample, filter mode */
int gstamd_audio_resampler_debug_get (GstAmdAudioResampler *resampler, int32_t *out, int max_out);
/* what the calling thread's last _resample, _resample_planes or _resample_many call did, 4 values: kernel launches issued, of those
 * launches of the interpolated LDS kernels, streams served by batched launches, streams gone one by one.  Returns 4. */
int gstamd_audio_resampler_debug_launches (int32_t *out, int max_out);
/* copies the [n_phases][n_taps] taps table (as doubles) out; returns number of values or < 0 */
long gstamd_audio_resampler_debug_taps (GstAmdAudioResampler *resampler, double *out, long max_out);

/* ---- GstAudioConverter (gst-libs/gst/audio/audio-converter.h:85-140, audio-converter.c) ------------------------------------------
 * The stages of gst_audio_converter_new's chain (audio-converter.c:708-1090) on the device: unpack -> S32 / F64, S32 -> F64
 * (convert_in), channel mix, resample, F64 -> S32 (convert_out), quantize (dither), pack.  Formats are GstAudioFormat values
 * (audio-format.h:80-130) - all 31 raw ones: S8 / U8; S16, S24_32 (24 bits in 4 bytes), S32, S24, S20 and S18 (in 3 bytes) signed and
 * unsigned, F32 and F64, each little- and big-endian.  A binding passes GST_AUDIO_INFO_FORMAT through.  Two formats that differ in byte
 * order only, with no mix and no rate change, are converted by swapping every sample's bytes (the reference's converter_endian):
 * nothing is unpacked, quantized or dithered, and floats pass with their denormals and NaN payloads. */
enum {
  GSTAMD_AFMT_S8 = 2, GSTAMD_AFMT_U8 = 3,
  GSTAMD_AFMT_S16LE = 4, GSTAMD_AFMT_S16BE = 5, GSTAMD_AFMT_U16LE = 6, GSTAMD_AFMT_U16BE = 7,
  GSTAMD_AFMT_S24_32LE = 8, GSTAMD_AFMT_S24_32BE = 9, GSTAMD_AFMT_U24_32LE = 10, GSTAMD_AFMT_U24_32BE = 11,
  GSTAMD_AFMT_S32LE = 12, GSTAMD_AFMT_S32BE = 13, GSTAMD_AFMT_U32LE = 14, GSTAMD_AFMT_U32BE = 15,
  GSTAMD_AFMT_S24LE = 16, GSTAMD_AFMT_S24BE = 17, GSTAMD_AFMT_U24LE = 18, GSTAMD_AFMT_U24BE = 19,
  GSTAMD_AFMT_S20LE = 20, GSTAMD_AFMT_S20BE = 21, GSTAMD_AFMT_U20LE = 22, GSTAMD_AFMT_U20BE = 23,
  GSTAMD_AFMT_S18LE = 24, GSTAMD_AFMT_S18BE = 25, GSTAMD_AFMT_U18LE = 26, GSTAMD_AFMT_U18BE = 27,
  GSTAMD_AFMT_F32LE = 28, GSTAMD_AFMT_F32BE = 29, GSTAMD_AFMT_F64LE = 30, GSTAMD_AFMT_F64BE = 31
};
/* GstAudioDitherMethod / GstAudioNoiseShapingMethod (audio-quantize.h:45-72) */
enum { GSTAMD_AUDIO_DITHER_NONE = 0, GSTAMD_AUDIO_DITHER_RPDF = 1, GSTAMD_AUDIO_DITHER_TPDF = 2, GSTAMD_AUDIO_DITHER_TPDF_HF = 3 };
#define GSTAMD_AUDIO_MAX_CHANNELS 8
#define GSTAMD_AUDIO_MAX_CHANNELS_WIDE 64       /* GstAudioInfo's own limit: gstamd_audio_converter_new_wide */
enum { GSTAMD_AUDIO_LAYOUT_INTERLEAVED = 0, GSTAMD_AUDIO_LAYOUT_NON_INTERLEAVED = 1 };  /* GstAudioLayout */

typedef struct GstAmdAudioInfo {
  int32_t format;               /* GSTAMD_AFMT_* */
  int32_t rate, channels;
  int32_t layout;               /* 0: the converter's layouts are arguments of gstamd_audio_converter_new_layouts, not this field */
  int32_t unpositioned;         /* GST_AUDIO_FLAG_UNPOSITIONED */
  int32_t position[GSTAMD_AUDIO_MAX_CHANNELS];  /* GstAudioChannelPosition values (audio-channels.h:101-133): NONE -3, MONO -2, FRONT_LEFT 0, FRONT_RIGHT 1, FRONT_CENTER 2, LFE1 3, REAR_LEFT 4, ... */
} GstAmdAudioInfo;

/* GstAmdAudioInfo with the 64 positions a GstAudioInfo holds (gstamd_audio_converter_new_wide) */
typedef struct GstAmdAudioInfoWide {
  int32_t format;
  int32_t rate, channels;
  int32_t layout;               /* 0, as in GstAmdAudioInfo */
  int32_t unpositioned;
  int32_t position[GSTAMD_AUDIO_MAX_CHANNELS_WIDE];
} GstAmdAudioInfoWide;

typedef struct GstAmdAudioConverterConfig {
  int32_t dither_method;        /* GstAudioConverter.dither-method (library default: none) */
  int32_t noise_shaping;        /* GstAudioConverter.noise-shaping-method (library default: NONE; 1 error-feedback, 2 simple, 3 medium, 4 high - one lane per channel walks the recurrence) */
  uint32_t dither_threshold;    /* GstAudioConverter.dither-threshold (20) */
  int32_t resampler_method;     /* GstAudioConverter.resampler-method (BLACKMAN_NUTTALL = 3) */
  int32_t has_resampler_options;
  GstAmdAudioResamplerOptions resampler_options;
  int32_t has_mix_matrix;       /* GstAudioConverter.mix-matrix: mix_matrix[out][in] as in the option (audio-converter.c:797-845) */
  float mix_matrix[GSTAMD_AUDIO_MAX_CHANNELS][GSTAMD_AUDIO_MAX_CHANNELS];
} GstAmdAudioConverterConfig;

typedef struct GstAmdAudioConverter GstAmdAudioConverter;

void gstamd_audio_converter_config_init (GstAmdAudioConverterConfig *config);
/* flags: GstAudioConverterFlags (audio-converter.h:99-103; 2 = VARIABLE_RATE).  NULL + *status on failure
 * (GSTAMD_ERR_UNSUPPORTED: the reference converts this, the GPU path does not yet - never a CPU fallback). */
GstAmdAudioConverter *gstamd_audio_converter_new (int flags, const GstAmdAudioInfo *in_info, const GstAmdAudioInfo *out_info,
    const GstAmdAudioConverterConfig *config, int *status);
/* gst_audio_converter_new with the layouts of the two GstAudioInfos given beside them.  in_info->layout and out_info->layout must be 0
 * here as in gstamd_audio_converter_new (which keeps refusing a non-zero one): the layouts are these two arguments; (.., 0, .., 0, ..)
 * makes the converter gstamd_audio_converter_new makes.  What a non-interleaved side changes: the passthrough and the
 * byte-swap shortcut need equal layouts; where the layouts differ the mix stage runs even with an identity matrix; the quantizer of a
 * non-interleaved output dithers and shapes plane after plane as ONE channel, as gst_audio_quantize_samples does. */
GstAmdAudioConverter *gstamd_audio_converter_new_layouts (int flags, const GstAmdAudioInfo *in_info, int in_layout,
    const GstAmdAudioInfo *out_info, int out_layout, const GstAmdAudioConverterConfig *config, int *status);
/* gstamd_audio_converter_new_layouts for 1 .. 64 channels on each side.  mix_matrix: NULL for the default matrix, else
 * out_info->channels rows of in_info->channels floats, [out][in] as the GstAudioConverter.mix-matrix option; config->has_mix_matrix must be 0
 * (its [8][8] array cannot hold the matrix).  The converter keeps its matrix in device memory and mixes a tile of frames through LDS; it
 * does so at 8 channels or fewer too, where it gives the bytes of the converter gstamd_audio_converter_new_layouts makes.  Every other entry
 * point works on it; gstamd_audio_converter_samples_planes takes up to 64 plane pointers. */
GstAmdAudioConverter *gstamd_audio_converter_new_wide (int flags, const GstAmdAudioInfoWide *in_info, int in_layout,
    const GstAmdAudioInfoWide *out_info, int out_layout, const GstAmdAudioConverterConfig *config, const float *mix_matrix, int *status);
void gstamd_audio_converter_free (GstAmdAudioConverter *convert);
void gstamd_audio_converter_reset (GstAmdAudioConverter *convert);
size_t gstamd_audio_converter_get_out_frames (GstAmdAudioConverter *convert, size_t in_frames);
size_t gstamd_audio_converter_get_in_frames (GstAmdAudioConverter *convert, size_t out_frames);
size_t gstamd_audio_converter_get_max_latency (GstAmdAudioConverter *convert);
int gstamd_audio_converter_is_passthrough (GstAmdAudioConverter *convert);
/* gst_audio_converter_samples (audio-converter.c:1545): in / out are device pointers to interleaved frames; in == NULL feeds
 * silence into the resampler (drain).  A non-interleaved side (gstamd_audio_converter_new_layouts) holds its channels one after the
 * other, in_frames (out_frames) samples apart, as in gstamd_audio_resampler_resample. */
int gstamd_audio_converter_samples (GstAmdAudioConverter *convert, int flags, const void *in, size_t in_frames, void *out, size_t out_frames,
    void *stream);
/* gst_audio_converter_samples' own argument shape: in[] / out[] hold ONE pointer for an interleaved side and `channels` pointers for a
 * non-interleaved one (any device addresses aligned to the sample size; planes need not be equally spaced); in == NULL feeds silence
 * into the resampler */
int gstamd_audio_converter_samples_planes (GstAmdAudioConverter *convert, int flags, const void *const in[], size_t in_frames,
    void *const out[], size_t out_frames, void *stream);
/* the mix matrix the converter uses, matrix[in][out] as GstAudioChannelMixer holds it; returns in_channels * out_channels */
int gstamd_audio_converter_get_mix_matrix (GstAmdAudioConverter *convert, float *matrix, int max);
/* n independent converters, one buffer each, in as few launches as their plans allow.  Outputs and converter states
 * are exactly those of n gstamd_audio_converter_samples calls made in array order.  No reference counterpart.
 * in[i] / out[i] are what gstamd_audio_converter_samples takes for converters[i]; in == NULL or in[i] == NULL feeds silence;
 * in_frames[i] == 0 skips that stream.  Everything is validated before anything is launched: a NULL converter, a NULL out[i] with
 * out_frames[i] > 0, a NULL input or in_frames[i] != out_frames[i] for a converter without a resampler return GSTAMD_ERR_INVALID with
 * nothing done.  Consecutive converters (up to 64) made with equal arguments - any constructor, layouts and channel count, the mix
 * matrix of a wide converter included; not a passthrough or a byte swap, non-NULL input, fewer than 2^30 frames - share one first
 * kernel, one gstamd_audio_resampler_resample_many, one second kernel and one noise shaping kernel; every other
 * one, and the same converter a second time, goes through the single-stream path in its place in the order.  The buffers of different
 * streams must not overlap. */
int gstamd_audio_converter_samples_many (int n, GstAmdAudioConverter *const *converters, int flags, const void *const *in,
    const size_t *in_frames, void *const *out, const size_t *out_frames, void *stream);
/* for tests: what the calling thread's last gstamd_audio_converter_samples_many did - { batched runs, streams served by batched runs,
 * streams gone one by one, launches of the batched converter kernels (the resampler's own not counted) }; returns 4 */
int gstamd_audio_converter_debug_many (int32_t *out, int max_out);

/* ---- audiomixer (gst-plugins-base/gst/audiomixer: gstaudiomixer.c, gstaudiomixerorc.orc) --------------------------------------------
 * The sum of many streams of one format into one buffer, as gst_audio_mixer_aggregate_one_buffer builds it pad after pad - here in ONE
 * launch for up to 64 inputs: every output sample is written once, its running sum kept in registers and taken in array (pad) order,
 * which the saturating integer adds make observable.  Per sample of an input that is not skipped: volume == 1.0 adds the sample
 * (audiomixer_orc_add_*); any other volume scales it first (audiomixer_orc_add_volume_*: S16 by (int) (volume * 2048) >> 11, S32 by
 * (int) (volume * 134217728) >> 27, both saturating; F32 by (float) volume, F64 by volume), with ORC's denormal flush around every
 * float operation and no fused multiply-add.  NaN payloads are not pinned.  DESIGN 3.9 has the table.
 * Formats: GSTAMD_AFMT_S16LE, _S32LE, _F32LE, _F64LE, interleaved.  The reference element also mixes S8, U8, U16LE and U32LE: those
 * return GSTAMD_ERR_UNSUPPORTED here, as does every other GSTAMD_AFMT_* value.  Callers convert first
 * (gstamd_audio_converter_samples_many) and mix on the same stream; no synchronisation is needed in between. */
typedef struct GstAmdAudioMixerInput {
  const void *data;     /* device pointer to the FIRST frame of this input that lands in the output; aligned to the sample size */
  uint64_t out_offset;  /* output frame at which that first frame lands */
  uint64_t frames;      /* frames contributed; out_offset + frames <= out_frames */
  double volume;        /* GstAudioMixerPad "volume", 0 .. 10 */
  int32_t mute;         /* GstAudioMixerPad "mute" */
  int32_t reserved;
} GstAmdAudioMixerInput;

/* out[0 .. out_frames) is written exactly once: frames no input covers are silence (all-zero bytes).  An input is skipped when it is
 * muted, its volume is below DBL_MIN (the reference's G_MINDOUBLE), it has no frames or data == NULL.  Inputs must not overlap `out`.
 * Asynchronous on `stream`.  GSTAMD_ERR_INVALID, with nothing launched: n_inputs < 0 (or inputs == NULL with n_inputs > 0), out == NULL
 * with out_frames > 0, a pointer not aligned to the sample size, out_offset + frames > out_frames, out_frames >= 2^30, channels outside
 * 1 .. 64, a volume that is NaN, negative or above 10.  Launches: one for up to 64 live inputs (none: one that writes silence); every
 * further 64 live inputs one more on the same stream, which starts from the output of the one before - the sum is sequential, so the
 * result is the same. */
int gstamd_audio_mixer_mix (int format, int channels, const GstAmdAudioMixerInput *inputs, int n_inputs,
    void *out, size_t out_frames, void *stream);
/* what the calling thread's last gstamd_audio_mixer_mix did:
 * { kernel launches, inputs mixed, inputs skipped (mute / volume / empty), 0 }; returns 4 */
int gstamd_audio_mixer_debug_launches (int32_t *out, int max_out);

/* ---- volume (gst-plugins-base/gst/volume: gstvolume.c, gstvolumeorc.orc) --------------------------------------------------------------
 * The element's sample loops on buffers that stay in device memory, many buffers a launch.  Two rules (DESIGN 3.10 has the tables):
 * (a) gains == NULL - a fixed volume, as volume_update_volume picks the loop (gstvolume.c): the volume is held as a float; mute or 0.0
 *     writes silence, (gint) (volume * 2048) == 2048 passes the bytes through, anything else runs volume_orc_process_int8 / _int16 /
 *     _int32 (and their _clamp forms), volume_process_int24 (_clamp), volume_orc_scalarmultiply_f32_ns / _f64_ns (gstvolumeorc.orc);
 * (b) gains != NULL - one double per frame, the value array a control binding fills, as volume_process_controlled_* applies it
 *     (gstvolume.c): 1 and 2 channels through volume_orc_process_controlled_*_1ch / _2ch, every other count through the plain C loops,
 *     which differ in rounding and in the denormal flush; mute turns every gain into +0.0 (volume_orc_prepare_volumes).
 * Integer results saturate; ORC's denormal flush is done with bit operations; no fused multiply-add.  NaN payloads are not pinned.
 * Formats: GSTAMD_AFMT_S8, _S16LE, _S24LE (3 bytes), _S32LE, _F32LE, _F64LE, interleaved - the six the element takes.  Every other
 * GSTAMD_AFMT_* value returns GSTAMD_ERR_UNSUPPORTED. */
typedef struct GstAmdAudioVolumeBuffer {
  const void *in;        /* device pointer; aligned to the sample size (S24: any byte address) */
  void *out;             /* == in: in place; else the two byte ranges must not overlap */
  uint64_t frames;
  double volume;         /* GstVolume "volume", 0 .. 10; ignored when gains != NULL */
  const double *gains;   /* NULL: rule (a); else device pointer to `frames` doubles, 8-byte aligned: rule (b) */
  int32_t mute, reserved;       /* GstVolume "mute" */
} GstAmdAudioVolumeBuffer;

/* volume_transform_ip on one buffer (gstvolume.c): gstamd_audio_volume_process_many with one entry */
int gstamd_audio_volume_process (int format, int channels, const void *in, void *out, size_t frames,
    double volume, int mute, const double *gains, void *stream);
/* The same on n buffers of one format and channel count (gstvolume.c volume_transform_ip, gstvolumeorc.orc).  A buffer that passes through in
 * place takes part in no launch; every other buffer - scaled, with gains, silenced, or passed through out of place as a copy - is one
 * descriptor of a launch, in array order, 64 descriptors per launch, every further 64 one more launch on the same stream.  A buffer with
 * frames == 0 does nothing.  Buffers of different entries must not overlap one another (not checked).  Asynchronous on `stream`.
 * GSTAMD_ERR_INVALID, with nothing launched and no byte written: channels outside 1 .. 64, frames >= 2^30, in or out NULL with
 * frames > 0, a misaligned pointer, in and out overlapping without being equal, a volume that is NaN, negative or above 10 (only when
 * gains == NULL), n < 0 (or buffers == NULL with n > 0).  All buffers are checked before the first launch. */
int gstamd_audio_volume_process_many (int format, int channels, const GstAmdAudioVolumeBuffer *buffers, int n, void *stream);
/* what the calling thread's last gstamd_audio_volume_process / _process_many did (gstvolume.c has no counterpart; for tests):
 * { kernel launches, buffers scaled (rule (a)'s formulas or rule (b)), buffers passed through, buffers silenced }; buffers without frames
 * are in none of the three; returns 4 */
int gstamd_audio_volume_debug_launches (int32_t *out, int max_out);

#ifdef __cplusplus
}
#endif
#endif /* GSTAMD_AUDIO_H */
