// tests/emu/emu_audio_handles.h - TEST INFRASTRUCTURE: the handles of emu_aconv_planes_new (emu_audio_planes.cpp) and emu_aconv_wide_new
// (emu_audio_wide.cpp), which emu_audio_many.cpp reads as well.
#pragma once
#include <vector>

#include "../../gstreamer_amd/csrc/audio_convert_plan.h"

struct EmuAConvPlanes {
  gstamd::AConvPlan plan;
  int in_layout = 0, out_layout = 0, flags = 0;
  GstAmdAudioInfo in, out;
  GstAmdAudioConverterConfig cfg;
  bool resample = false, passthrough = false;
  void *resampler = nullptr;
  gstamd::AConvDitherState dither = { 0xc2d6038fu, 0u, 0 };
  gstamd::AConvJump jump;
  std::vector<int32_t> hist = std::vector<int32_t> (8 * GSTAMD_AUDIO_MAX_CHANNELS, 0);
};

struct EmuAConvWide {
  gstamd::AConvWidePlan plan;
  int in_layout = 0, out_layout = 0, flags = 0, in_rate = 0, out_rate = 0;
  GstAmdAudioConverterConfig cfg;
  bool resample = false, passthrough = false;
  void *resampler = nullptr;
  gstamd::AConvDitherState dither = { 0xc2d6038fu, 0u, 0 };
  gstamd::AConvJump jump;
  std::vector<int32_t> hist = std::vector<int32_t> (8 * GSTAMD_AUDIO_MAX_CHANNELS_WIDE, 0);
};
