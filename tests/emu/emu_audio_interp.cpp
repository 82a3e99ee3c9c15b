// tests/emu/emu_audio_interp.cpp - TEST INFRASTRUCTURE: the grids of k_fir_interp_lds and k_fir_interp_lds_many (and, for streams that
// change mode and arrays that mix modes, of k_fir_lds / k_fir_lds_many) walked on the host block by block and lane by lane over the
// body functions of audio_device.h, with the library's own host bookkeeping (plan_audio_resampler, audio_step) and the same fit rule
// (fir_interp_lds_bytes <= FIR_LDS_BUDGET).  Mirrors run_resample / run_many / gstamd_audio_resampler_resample_many of
// audio_kernels.hip; emu_interp_launches is gstamd_audio_resampler_debug_launches.  The LDS of a workgroup is one byte array laid out
// as the kernel lays it out, filled with 0x5a before every block: what a lane reads without anybody having staged it shows in the bytes.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gstreamer_amd/csrc/audio_device.h"
#include "../../gstreamer_amd/csrc/audio_taps.h"

using namespace gstamd;

namespace {

struct EmuInterp {
  AudioPlan plan;
  AudioState st;
  std::vector<uint8_t> hist;
};

thread_local int32_t launches[4] = { 0, 0, 0, 0 };

bool knob (const char *name) { return getenv (name) != nullptr; }

int interp_of (const AudioPlan &pl)
{
  return pl.filter_mode == GSTAMD_AUDIO_FILTER_MODE_INTERPOLATED && pl.method != GSTAMD_AUDIO_RESAMPLER_METHOD_NEAREST ?
      (pl.filter_interpolation == GSTAMD_AUDIO_FILTER_INTERPOLATION_CUBIC ? 2 : 1) : 0;
}

// make_fir_params
FirParams make_params (const AudioPlan &pl, const AudioStep &s, bool in_null, long long in_stride, long long out_stride)
{
  FirParams p;
  memset (&p, 0, sizeof (p));
  p.channels = pl.channels;
  p.n_taps_padded = pl.taps_stride;
  p.interp = interp_of (pl);
  p.oversample = pl.oversample;
  p.nearest = (pl.method == GSTAMD_AUDIO_RESAMPLER_METHOD_NEAREST || pl.in_rate == pl.out_rate) ? 1 : 0;
  p.samp_inc = pl.samp_inc;
  p.samp_frac = pl.samp_frac;
  p.out_rate = pl.out_rate;
  p.samp_index0 = s.samp_index0;
  p.samp_phase0 = s.samp_phase0;
  p.hist_frames = s.hist_frames;
  p.total_frames = s.total_frames;
  p.in_is_null = in_null;
  p.in_plane_stride = pl.in_planar ? in_stride : 0;
  p.out_plane_stride = pl.out_planar ? out_stride : 0;
  return p;
}

// LDS bytes of the plan's staged kernel (FULL: k_fir_lds's, INTERPOLATED: k_fir_interp_lds's), 0 for plans without one
size_t lds_bytes (const AudioPlan &pl, FirLdsGeom *gf, FirInterpGeom *gi)
{
  if (pl.method == GSTAMD_AUDIO_RESAMPLER_METHOD_NEAREST || pl.in_rate == pl.out_rate)
    return 0;
  const int interp = interp_of (pl);
  if (interp)
    return fir_interp_lds_bytes (pl.bps, pl.channels, pl.taps_stride, pl.samp_inc, interp, pl.oversample, gi);
  gf->row_stride = pl.taps_stride + 4;
  gf->win_frames = fir_lds_win_frames (pl.samp_inc, pl.taps_stride);
  return ((size_t) FIR_LDS_FRAMES * gf->row_stride + (size_t) pl.channels * gf->win_frames) * (size_t) pl.bps + 2 * FIR_LDS_FRAMES * sizeof (int);
}

// one workgroup of fir_lds_block (p.interp == 0) / fir_interp_lds_block
template <typename T>
void walk_block (const FirParams &p, const FirLdsGeom &gf, const FirInterpGeom &gi, const T *hist, const T *in, const T *table, T *out, long long n_out,
    int fir_blocks, T *new_hist, long long src_start, long long moved, long long keep, int bx, std::vector<uint64_t> &lds)
{
  typedef typename Acc<T>::type A;
  if (bx >= fir_blocks) {
    for (int tid = 0; tid < 256; tid++) {
      const long long i = (long long) (bx - fir_blocks) * 256 + tid;
      if (i < keep * p.channels)
        new_hist[i] = history_sample<T> (p, hist, in, src_start, moved, i / p.channels, (int) (i % p.channels));
    }
    return;
  }
  memset (lds.data (), 0x5a, lds.size () * sizeof (uint64_t));
  const long long jb = (long long) bx * FIR_LDS_FRAMES;
  const int nj = n_out - jb < FIR_LDS_FRAMES ? (int) (n_out - jb) : FIR_LDS_FRAMES;
  A r[256];
  if (p.interp) {
    T *tab = (T *) lds.data (), *win = tab + (size_t) gi.n_rows * gi.row_stride, *ic = win + (size_t) p.channels * gi.win_frames;
    int *pos = (int *) (ic + 4 * FIR_LDS_FRAMES);
    for (int tid = 0; tid < 256; tid++) {          /* no barrier between these four in the kernel: lane after lane */
      fir_lds_positions (p, jb, nj, pos, tid, 256);
      fir_interp_coeffs<T> (p, nj, pos, ic, tid, 256);
      fir_interp_stage_table<T> (p, gi, table, tab, tid, 256);
      fir_lds_stage_window<T> (p, gi.win_frames, hist, in, jb, nj, win, tid, 256);
    }
    for (int c = 0; c < p.channels; c++) {
      for (int tid = 0; tid < 256; tid++) {
        const int fr = tid >> 2, q = tid & 3, frc = fr < nj ? fr : nj - 1;
        r[tid] = fir_interp_partial<T> (p, gi, pos, tab, win, frc, q, c);
      }
      for (int tid = 0; tid < 256; tid++) {
        const int fr = tid >> 2, q = tid & 3, base = tid & ~3;
        if (fr < nj && q == (c & 3))
          out[fir_out_index (p, jb + fr, c)] = fir_interp_combine<T> (p, r[base], r[base + 1], r[base + 2], r[base + 3], ic + 4 * fr);
      }
    }
    return;
  }
  T *rows = (T *) lds.data (), *win = rows + FIR_LDS_FRAMES * gf.row_stride;
  int *pos = (int *) (win + (size_t) p.channels * gf.win_frames);
  for (int tid = 0; tid < 256; tid++)
    fir_lds_positions (p, jb, nj, pos, tid, 256);
  for (int tid = 0; tid < 256; tid++)
    fir_lds_stage<T> (p, gf, hist, in, table, jb, nj, pos, rows, win, tid, 256);
  for (int c = 0; c < p.channels; c++) {
    for (int tid = 0; tid < 256; tid++) {
      const int fr = tid >> 2, q = tid & 3, frc = fr < nj ? fr : nj - 1;
      r[tid] = fir_lds_partial<T> (p, gf, pos, rows, win, frc, q, c);
    }
    for (int tid = 0; tid < 256; tid++) {
      const int fr = tid >> 2, q = tid & 3, base = tid & ~3;
      if (fr < nj && q == (c & 3))
        out[fir_out_index (p, jb + fr, c)] = fir_lds_combine<T> (r[base], r[base + 1], r[base + 2], r[base + 3]);
    }
  }
}

// run_resample
template <typename T>
void run_one (EmuInterp *r, const void *in, size_t in_frames, void *out, size_t out_frames)
{
  const AudioPlan &pl = r->plan;
  const AudioStep s = audio_step (pl, &r->st, in_frames, out_frames);
  launches[3]++;
  if (s.skipped_all)
    return;
  const FirParams p = make_params (pl, s, in == nullptr, (long long) in_frames, (long long) out_frames);
  const T *hist = (const T *) r->hist.data ();
  std::vector<uint8_t> nh ((size_t) (s.keep + 1) * pl.channels * sizeof (T));
  FirLdsGeom gf = { 0, 0 };
  FirInterpGeom gi = { 0, 0, 0 };
  const size_t lds = lds_bytes (pl, &gf, &gi);
  if (s.run_fir && !p.nearest && !knob ("GSTAMD_NO_FIR_LDS") && lds <= FIR_LDS_BUDGET) {
    std::vector<uint64_t> mem ((lds + 7) / 8);
    const int fir_blocks = (int) ((s.n_out + FIR_LDS_FRAMES - 1) / FIR_LDS_FRAMES);
    const int hist_blocks = s.keep > 0 ? (int) ((s.keep * pl.channels + 255) / 256) : 0;
    for (int bx = 0; bx < fir_blocks + hist_blocks; bx++)
      walk_block<T> (p, gf, gi, hist, (const T *) in, (const T *) pl.table.data (), (T *) out, s.n_out, fir_blocks, (T *) nh.data (), s.src_start, s.moved,
          s.keep, bx, mem);
    launches[0]++;
    launches[1] += p.interp ? 1 : 0;
    r->hist.swap (nh);
    return;
  }
  if (s.run_fir) {                              /* k_fir */
    for (long long j = 0; j < s.n_out; j++)
      for (int c = 0; c < pl.channels; c++)
        ((T *) out)[fir_out_index (p, j, c)] = fir_output<T> (p, hist, (const T *) in, (const T *) pl.table.data (), j, c);
    launches[0]++;
  }
  if (s.keep > 0) {                             /* k_history */
    for (long long i = 0; i < s.keep; i++)
      for (int c = 0; c < pl.channels; c++)
        ((T *) nh.data ())[i * pl.channels + c] = history_sample<T> (p, hist, (const T *) in, s.src_start, s.moved, i, c);
    launches[0]++;
  }
  r->hist.swap (nh);
}

void resample_one (EmuInterp *r, const void *in, size_t in_frames, void *out, size_t out_frames)
{
  switch (r->plan.format) {
    case GSTAMD_AUDIO_FORMAT_S16: run_one<int16_t> (r, in, in_frames, out, out_frames); break;
    case GSTAMD_AUDIO_FORMAT_S32: run_one<int32_t> (r, in, in_frames, out, out_frames); break;
    case GSTAMD_AUDIO_FORMAT_F32: run_one<float> (r, in, in_frames, out, out_frames); break;
    default: run_one<double> (r, in, in_frames, out, out_frames); break;
  }
}

// run_many
template <typename T>
void run_many (int n, EmuInterp *const *rs, const void *const *in, const size_t *in_frames, void *const *out, const size_t *out_frames)
{
  const AudioPlan &pl = rs[0]->plan;
  FirMany many;
  memset ((void *) &many, 0, sizeof (many));
  AudioStep first;
  memset (&first, 0, sizeof (first));
  int max_blocks = 0, live = 0;
  launches[2] += n;
  std::vector<std::vector<uint8_t>> nh ((size_t) n);
  std::vector<EmuInterp *> owner;
  for (int i = 0; i < n; i++) {
    EmuInterp *r = rs[i];
    const AudioStep s = audio_step (r->plan, &r->st, in_frames[i], out_frames[i]);
    if (s.skipped_all)
      continue;
    nh[(size_t) live].assign ((size_t) (s.keep + 1) * pl.channels * sizeof (T), 0);
    FirManyStream &m = many.s[live];
    m.hist = r->hist.data ();
    m.new_hist = nh[(size_t) live].data ();
    m.in = in[i];
    m.out = out[i];
    m.samp_index0 = (int) s.samp_index0;
    m.samp_phase0 = s.samp_phase0;
    m.hist_frames = (int) s.hist_frames;
    m.in_frames = (int) (s.total_frames - s.hist_frames);
    m.n_out = s.run_fir ? (int) s.n_out : 0;
    const int blocks = (int) ((m.n_out + FIR_LDS_FRAMES - 1) / FIR_LDS_FRAMES) + (s.keep > 0 ? (int) ((s.keep * pl.channels + 255) / 256) : 0);
    max_blocks = blocks > max_blocks ? blocks : max_blocks;
    owner.push_back (r);
    live++;
    first = s;
  }
  if (!live || !max_blocks) {
    for (int y = 0; y < live; y++)
      owner[(size_t) y]->hist.swap (nh[(size_t) y]);
    return;
  }
  const FirParams shared = make_params (pl, first, false, 1, 1);
  FirLdsGeom gf = { 0, 0 };
  FirInterpGeom gi = { 0, 0, 0 };
  const size_t lds = lds_bytes (pl, &gf, &gi);
  std::vector<uint64_t> mem ((lds + 7) / 8);
  for (int y = 0; y < live; y++)                /* blockIdx.y = stream */
    for (int bx = 0; bx < max_blocks; bx++) {
      const FirManyStream &m = many.s[y];
      FirParams p;
      FirManyWork w;
      fir_many_stream (shared, m, &p, &w);
      if (bx >= w.fir_blocks + w.hist_blocks)
        continue;
      walk_block<T> (p, gf, gi, (const T *) m.hist, (const T *) m.in, (const T *) pl.table.data (), (T *) m.out, m.n_out, w.fir_blocks, (T *) m.new_hist,
          w.src_start, w.moved, w.keep, bx, mem);
    }
  launches[0]++;
  launches[1] += shared.interp ? 1 : 0;
  for (int y = 0; y < live; y++)
    owner[(size_t) y]->hist.swap (nh[(size_t) y]);
}

}  // namespace

extern "C" {

void *emu_interp_new (int method, int flags, int format, int channels, int in_rate, int out_rate, const GstAmdAudioResamplerOptions *options, int *status)
{
  EmuInterp *r = new EmuInterp ();
  std::string e;
  const int st = plan_audio_resampler (method, flags, format, channels, in_rate, out_rate, options, &r->plan, &e);
  if (status)
    *status = st;
  if (st != GSTAMD_OK) {
    delete r;
    return nullptr;
  }
  audio_state_reset (r->plan, &r->st);
  r->hist.assign ((size_t) (r->plan.n_taps + 8) * channels * r->plan.bps, 0);
  return r;
}

void emu_interp_free (void *h) { delete (EmuInterp *) h; }
size_t emu_interp_get_out_frames (void *h, size_t in_frames) { EmuInterp *r = (EmuInterp *) h; return audio_get_out_frames (r->plan, r->st, in_frames); }
size_t emu_interp_get_max_latency (void *h) { return (size_t) (((EmuInterp *) h)->plan.n_taps / 2); }
int emu_interp_filter_mode (void *h) { return ((EmuInterp *) h)->plan.filter_mode; }

// LDS bytes the plan's staged kernel would need (compare with 64 * 1024), 0 for a plan without one
size_t emu_interp_lds_bytes (void *h)
{
  FirLdsGeom gf;
  FirInterpGeom gi;
  return lds_bytes (((EmuInterp *) h)->plan, &gf, &gi);
}

// emu_audio_update (emu_audio.cpp) on this file's handle
int emu_interp_update (void *h, int in_rate, int out_rate, const GstAmdAudioResamplerOptions *options)
{
  EmuInterp *r = (EmuInterp *) h;
  AudioHistoryShift shift;
  std::string e;
  const size_t old_avail = r->st.samples_avail + (size_t) r->st.samp_index;
  const int st = audio_update (&r->plan, &r->st, in_rate, out_rate, options, &shift, &e);
  if (st != GSTAMD_OK)
    return st;
  const size_t fbytes = (size_t) r->plan.channels * r->plan.bps;
  if (r->hist.size () > old_avail * fbytes)
    r->hist.resize (old_avail * fbytes);
  audio_history_shift (shift, fbytes, &r->hist);
  r->hist.resize (r->hist.size () + 8 * fbytes, 0);
  return st;
}

void emu_interp_resample (void *h, const void *in, size_t in_frames, void *out, size_t out_frames)
{
  memset (launches, 0, sizeof (launches));
  resample_one ((EmuInterp *) h, in, in_frames, out, out_frames);
}

// gstamd_audio_resampler_resample_many
int emu_interp_resample_many (int n, void *const *handles, const void *const *in, const size_t *in_frames, void *const *out, const size_t *out_frames)
{
  memset (launches, 0, sizeof (launches));
  if (n < 0 || (n > 0 && (!handles || !in_frames || !out || !out_frames)))
    return GSTAMD_ERR_INVALID;
  for (int i = 0; i < n; i++)
    if (!handles[i] || (out_frames[i] > 0 && !out[i]))
      return GSTAMD_ERR_INVALID;
  EmuInterp *const *rs = (EmuInterp *const *) handles;
  int done = 0;
  while (done < n) {
    EmuInterp *r0 = rs[done];
    const AudioPlan &p0 = r0->plan;
    const bool staged = p0.method != GSTAMD_AUDIO_RESAMPLER_METHOD_NEAREST && p0.in_rate != p0.out_rate && !knob ("GSTAMD_NO_FIR_LDS") &&
        !knob ("GSTAMD_NO_FIR_MANY");
    int run = 1;
    while (staged && done + run < n && run < GSTAMD_AUDIO_MANY_MAX) {
      EmuInterp *r = rs[done + run];
      bool dup = false;
      for (int k = 0; k < run; k++)
        dup = dup || rs[done + k] == r;
      if (dup)
        break;
      const AudioPlan &p = r->plan;
      if (p.format != p0.format || p.channels != p0.channels || p.in_rate != p0.in_rate || p.out_rate != p0.out_rate || p.n_taps != p0.n_taps ||
          p.taps_stride != p0.taps_stride || p.in_planar != p0.in_planar || p.out_planar != p0.out_planar || p.method != p0.method ||
          p.filter_mode != p0.filter_mode || p.filter_interpolation != p0.filter_interpolation || p.oversample != p0.oversample || p.table != p0.table)
        break;
      run++;
    }
    bool fits = staged && run > 1;
    for (int k = 0; fits && k < run; k++)
      fits = in && in[done + k] && in_frames[done + k] < (1u << 30) && out_frames[done + k] < (1u << 30);
    if (fits) {
      FirLdsGeom gf;
      FirInterpGeom gi;
      fits = lds_bytes (p0, &gf, &gi) <= FIR_LDS_BUDGET;
    }
    if (!fits) {
      resample_one (r0, in ? in[done] : nullptr, in_frames[done], out[done], out_frames[done]);
      done++;
      continue;
    }
    switch (p0.format) {
      case GSTAMD_AUDIO_FORMAT_S16: run_many<int16_t> (run, rs + done, in + done, in_frames + done, out + done, out_frames + done); break;
      case GSTAMD_AUDIO_FORMAT_S32: run_many<int32_t> (run, rs + done, in + done, in_frames + done, out + done, out_frames + done); break;
      case GSTAMD_AUDIO_FORMAT_F32: run_many<float> (run, rs + done, in + done, in_frames + done, out + done, out_frames + done); break;
      default: run_many<double> (run, rs + done, in + done, in_frames + done, out + done, out_frames + done); break;
    }
    done += run;
  }
  return GSTAMD_OK;
}

// gstamd_audio_resampler_debug_launches
int emu_interp_launches (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = launches[i];
  return 4;
}

}  // extern "C"
