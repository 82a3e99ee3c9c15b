// audio_volume.hip - gstamd_audio_volume_process / _process_many: the volume element's sample loops, up to 64 buffers a launch of
// k_audio_volume.  The plan (what each buffer needs, the groups of 64, the grid) and the body of a lane are
// audio_volume_device.h's, which tests/emu runs on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gstamd_audio.h"
#include "../../include/gstamd_video.h"
#include "audio_volume_device.h"

using namespace gstamd;

extern "C" void gstamd_internal_set_error (const char *msg);

static_assert (sizeof (AVolBuf) == 48 && sizeof (AVolArgs) <= 4096, "the descriptors of a launch travel in the kernel arguments");

// blockIdx.y: the buffer; blockIdx.x: a grid-stride walk over its pieces, a lane each; no LDS, no atomics, one store per piece
template <typename T>
__global__ __launch_bounds__ (AVOL_LANES) void k_audio_volume (AVolArgs a)
{
  const AVolBuf b = a.buf[blockIdx.y];
  const uint64_t pieces = avol_buffer_pieces<T> (b, a.channels);
  for (uint64_t q0 = (uint64_t) blockIdx.x * AVOL_LANES; q0 < pieces; q0 += (uint64_t) gridDim.x * AVOL_LANES)
    avol_lane<T> (b, a.channels, q0, (int) threadIdx.x);
}

static thread_local int32_t avol_debug[4] = { 0, 0, 0, 0 };

extern "C" {

int gstamd_audio_volume_process_many (int format, int channels, const GstAmdAudioVolumeBuffer *buffers, int n, void *stream_)
{
  hipStream_t stream = (hipStream_t) stream_;
  const int status = avol_run (format, channels, buffers, n, avol_debug, [&](const AVolArgs &a, unsigned grid) {
    const dim3 g (grid, (unsigned) a.n), l (AVOL_LANES);
    switch (format) {
      case GSTAMD_AFMT_S8: k_audio_volume<int8_t><<<g, l, 0, stream>>> (a); break;
      case GSTAMD_AFMT_S16LE: k_audio_volume<int16_t><<<g, l, 0, stream>>> (a); break;
      case GSTAMD_AFMT_S24LE: k_audio_volume<AVolS24><<<g, l, 0, stream>>> (a); break;
      case GSTAMD_AFMT_S32LE: k_audio_volume<int32_t><<<g, l, 0, stream>>> (a); break;
      case GSTAMD_AFMT_F32LE: k_audio_volume<float><<<g, l, 0, stream>>> (a); break;
      default: k_audio_volume<double><<<g, l, 0, stream>>> (a); break;
    }
    return hipGetLastError () == hipSuccess;
  });
  if (status != GSTAMD_OK)
    gstamd_internal_set_error (status == GSTAMD_ERR_HIP ? "audio volume: kernel launch" :
        status == GSTAMD_ERR_UNSUPPORTED ? "audio volume: format not built (S8, S16LE, S24LE, S32LE, F32LE, F64LE are)" : "audio volume: invalid argument");
  return status;
}

int gstamd_audio_volume_process (int format, int channels, const void *in, void *out, size_t frames, double volume, int mute,
    const double *gains, void *stream)
{
  GstAmdAudioVolumeBuffer b;
  b.in = in;
  b.out = out;
  b.frames = (uint64_t) frames;
  b.volume = volume;
  b.gains = gains;
  b.mute = mute;
  b.reserved = 0;
  return gstamd_audio_volume_process_many (format, channels, &b, 1, stream);
}

int gstamd_audio_volume_debug_launches (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = avol_debug[i];
  return 4;
}

}  // extern "C"
