// tests/emu/emu_audio_volume.cpp - TEST INFRASTRUCTURE: gstamd_audio_volume_process_many on the host the way the device runs
// it - the library's own launch plan (avol_run of audio_volume_device.h: the refusals, what each buffer needs, the groups of 64, the grid),
// and for every launch a loop over the grid: each buffer's workgroups, their grid-stride walk, 256 lanes, through the body k_audio_volume
// calls (avol_lane).  Mirrors audio_volume.hip; the buffers are host pointers.
#include <cstdint>

#include "../../gstreamer_amd/csrc/audio_volume_device.h"

using namespace gstamd;

namespace {

thread_local int32_t vol_debug[4] = { 0, 0, 0, 0 };

// k_audio_volume<T><<<dim3 (grid, a.n), 256>>> (a)
template <typename T> void launch (const AVolArgs &a, unsigned grid)
{
  for (int y = 0; y < a.n; y++) {
    const AVolBuf b = a.buf[y];
    const uint64_t pieces = avol_buffer_pieces<T> (b, a.channels);
    for (unsigned block = 0; block < grid; block++)
      for (uint64_t q0 = (uint64_t) block * AVOL_LANES; q0 < pieces; q0 += (uint64_t) grid * AVOL_LANES)
        for (int lane = 0; lane < AVOL_LANES; lane++)
          avol_lane<T> (b, a.channels, q0, lane);
  }
}

}  // namespace

extern "C" {

int emu_audio_volume_process_many (int format, int channels, const GstAmdAudioVolumeBuffer *buffers, int n, void *stream)
{
  (void) stream;
  return avol_run (format, channels, buffers, n, vol_debug, [&](const AVolArgs &a, unsigned grid) {
    switch (format) {
      case GSTAMD_AFMT_S8: launch<int8_t> (a, grid); break;
      case GSTAMD_AFMT_S16LE: launch<int16_t> (a, grid); break;
      case GSTAMD_AFMT_S24LE: launch<AVolS24> (a, grid); break;
      case GSTAMD_AFMT_S32LE: launch<int32_t> (a, grid); break;
      case GSTAMD_AFMT_F32LE: launch<float> (a, grid); break;
      default: launch<double> (a, grid); break;
    }
    return true;
  });
}

int emu_audio_volume_debug_launches (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = vol_debug[i];
  return 4;
}

}  // extern "C"
