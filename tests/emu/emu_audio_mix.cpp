// tests/emu/emu_audio_mix.cpp - TEST INFRASTRUCTURE: gstamd_audio_mixer_mix on the host the way the device runs it - the
// library's own launch plan (amix_run of audio_mix_device.h: the refusals, which inputs are live, the groups of 64, the grid), and for
// every launch a loop over the grid: each workgroup's grid-stride walk, 256 lanes, through the body k_audio_mix calls (amix_lane).
// Mirrors audio_mix.hip; the buffers are host pointers.
#include <cstdint>

#include "../../gstreamer_amd/csrc/audio_mix_device.h"

using namespace gstamd;

namespace {

thread_local int32_t mix_debug[4] = { 0, 0, 0, 0 };

// k_audio_mix<T><<<grid, 256>>> (a)
template <typename T> void launch (const AMixArgs &a, unsigned grid)
{
  const uint64_t pieces = amix_pieces (a.samples, a.lead, (int) sizeof (T));
  for (unsigned block = 0; block < grid; block++)
    for (uint64_t q0 = (uint64_t) block * AMIX_LANES; q0 < pieces; q0 += (uint64_t) grid * AMIX_LANES)
      for (int lane = 0; lane < AMIX_LANES; lane++)
        amix_lane<T> (a, q0, lane);
}

}  // namespace

extern "C" {

int emu_audio_mixer_mix (int format, int channels, const GstAmdAudioMixerInput *inputs, int n_inputs, void *out, size_t out_frames, void *stream)
{
  (void) stream;
  return amix_run (format, channels, inputs, n_inputs, out, out_frames, mix_debug, [&](const AMixArgs &a, unsigned grid) {
    switch (format) {
      case GSTAMD_AFMT_S16LE: launch<int16_t> (a, grid); break;
      case GSTAMD_AFMT_S32LE: launch<int32_t> (a, grid); break;
      case GSTAMD_AFMT_F32LE: launch<float> (a, grid); break;
      default: launch<double> (a, grid); break;
    }
    return true;
  });
}

int emu_audio_mixer_debug_launches (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = mix_debug[i];
  return 4;
}

}  // extern "C"
