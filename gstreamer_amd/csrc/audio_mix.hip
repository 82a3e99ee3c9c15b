// audio_mix.hip - gstamd_audio_mixer_mix: up to 64 streams summed into one buffer by one launch of k_audio_mix.  The plan
// (which inputs are live, the groups of 64, the grid) and the body of a lane are audio_mix_device.h's, which tests/emu runs on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/gstamd_audio.h"
#include "../../include/gstamd_video.h"
#include "audio_mix_device.h"

using namespace gstamd;

extern "C" void gstamd_internal_set_error (const char *msg);

static_assert (sizeof (AMixIn) == 32 && sizeof (AMixArgs) <= 4096, "the descriptors of a launch travel in the kernel arguments");

// a lane per aligned 16-byte piece of the output; no LDS, no atomics, one store per piece
template <typename T>
__global__ __launch_bounds__ (AMIX_LANES) void k_audio_mix (AMixArgs a)
{
  const uint64_t pieces = amix_pieces (a.samples, a.lead, (int) sizeof (T));
  for (uint64_t q0 = (uint64_t) blockIdx.x * AMIX_LANES; q0 < pieces; q0 += (uint64_t) gridDim.x * AMIX_LANES)
    amix_lane<T> (a, q0, (int) threadIdx.x);
}

static thread_local int32_t amix_debug[4] = { 0, 0, 0, 0 };

extern "C" {

int gstamd_audio_mixer_mix (int format, int channels, const GstAmdAudioMixerInput *inputs, int n_inputs, void *out, size_t out_frames, void *stream_)
{
  hipStream_t stream = (hipStream_t) stream_;
  const int status = amix_run (format, channels, inputs, n_inputs, out, out_frames, amix_debug, [&](const AMixArgs &a, unsigned grid) {
    switch (format) {
      case GSTAMD_AFMT_S16LE: k_audio_mix<int16_t><<<dim3 (grid), dim3 (AMIX_LANES), 0, stream>>> (a); break;
      case GSTAMD_AFMT_S32LE: k_audio_mix<int32_t><<<dim3 (grid), dim3 (AMIX_LANES), 0, stream>>> (a); break;
      case GSTAMD_AFMT_F32LE: k_audio_mix<float><<<dim3 (grid), dim3 (AMIX_LANES), 0, stream>>> (a); break;
      default: k_audio_mix<double><<<dim3 (grid), dim3 (AMIX_LANES), 0, stream>>> (a); break;
    }
    return hipGetLastError () == hipSuccess;
  });
  if (status != GSTAMD_OK)
    gstamd_internal_set_error (status == GSTAMD_ERR_HIP ? "audio mixer: kernel launch" :
        status == GSTAMD_ERR_UNSUPPORTED ? "audio mixer: format not built (S16LE, S32LE, F32LE, F64LE are)" : "audio mixer: invalid argument");
  return status;
}

int gstamd_audio_mixer_debug_launches (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = amix_debug[i];
  return 4;
}

}  // extern "C"
