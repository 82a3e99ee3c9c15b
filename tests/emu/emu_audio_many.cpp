// tests/emu/emu_audio_many.cpp - TEST INFRASTRUCTURE: gstamd_audio_converter_samples_many on the host the way the
// device runs it.  The call itself - the refusals, the walk with aconv_many_run_length, the stages of a batched run, the table entries, the
// counters - is aconv_many_samples of audio_convert_plan.h, the function the library calls; this file is its host backend: for every
// batched launch a loop over the grid through the body the kernel calls - k_aconv_pre_many / _pre_planes_many / _pre_mix_many /
// k_aconv_wide_mix_many (two phases around its barrier, a host "LDS" of the kernel's size), k_aconv_post_many / _post_planes_many,
// k_aconv_shape_many / _shape_planes_many (64 lanes, lane = stream).  Prefix "emu_aconv_many_".
//
// The converters are the emulator's existing handles, told apart in kind[]: 0 of emu_aconv_planes_new (emu_audio_planes.cpp: every
// converter of at most 8 channels), 1 of emu_aconv_wide_new (emu_audio_wide.cpp), 3 the latter with a resampler inside.  A stream that is
// not batched goes through its own emulator's emu_aconv_*_samples.
#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>

#include "../../gstreamer_amd/csrc/audio_convert_plan.h"
#include "emu_audio_handles.h"

using namespace gstamd;

extern "C" {
void emu_audio_resample (void *h, const void *in, size_t in_frames, void *out, size_t out_frames);
void emu_aconv_planes_samples (void *h, uint8_t *in, size_t in_frames, uint8_t *out, size_t out_frames);
void emu_aconv_wide_samples (void *h, uint8_t *in, size_t in_frames, uint8_t *out, size_t out_frames);
}

namespace {

thread_local int32_t many_debug[4] = { 0, 0, 0, 0 };

struct EmuManyBackend {
  void *const *convs;
  const int *kind;                              // NULL: all 0
  std::deque<std::vector<uint8_t>> pool;        // the buffers of the run under way

  bool has_convs () const { return convs != nullptr; }

  AConvManyConv conv (int i) const
  {
    void *h = convs[i];
    if (!h)
      return {};
    if (kind && (kind[i] & 1)) {
      EmuAConvWide *c = (EmuAConvWide *) h;
      return { h, &c->plan.s, &c->plan, true, c->passthrough, c->in_layout, c->out_layout, c->resampler, &c->dither, &c->jump, c->hist.data (), &c->jump,
        { c->plan.m.data (), c->plan.mi.data (), c->plan.use.data () } };
    }
    EmuAConvPlanes *c = (EmuAConvPlanes *) h;
    return { h, &c->plan, nullptr, false, c->passthrough, c->in_layout, c->out_layout, c->resampler, &c->dither, &c->jump, c->hist.data (), &c->jump,
      { nullptr, nullptr, nullptr } };
  }

  int fail (int code, const char *) { return code; }

  int single (const AConvManyConv &c, const void *in, size_t in_frames, void *out, size_t out_frames)
  {
    (c.wide ? emu_aconv_wide_samples : emu_aconv_planes_samples) (c.h, (uint8_t *) in, in_frames, (uint8_t *) out, out_frames);
    return GSTAMD_OK;
  }

  uint8_t *fresh (size_t bytes, uint8_t fill)
  {
    if (!bytes)
      return nullptr;
    pool.emplace_back (bytes, fill);
    return pool.back ().data ();
  }

  int buffers (const AConvManyConv &, size_t mid_a_bytes, size_t mid_b_bytes, size_t q_bytes, AConvManyBuffers *b)
  {
    *b = { fresh (mid_a_bytes, 0xcd), fresh (mid_b_bytes, 0xcd), (int32_t *) fresh (q_bytes, 0) };
    return GSTAMD_OK;
  }

  static size_t grid (size_t lanes) { return ((lanes + 255) / 256) * 256; }

  void pre (const AConvPlan &p, const AConvManyPreTable &t, size_t lanes, int run)      /* blockIdx.y = stream */
  {
#define PRE(K) for (int y = 0; y < run; y++) for (size_t x = 0; x < grid (lanes); x++) aconv_pre_many_lane<K> (p, t.s[y], x)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }

  void pre_planes (const AConvPlan &p, const AConvManyPrePlanesTable &t, size_t lanes, int run)        /* blockIdx.y = output channel, blockIdx.z = stream */
  {
#define PRE(K) for (int z = 0; z < run; z++) for (int y = 0; y < p.out_ch; y++) for (size_t x = 0; x < grid (lanes); x++) aconv_pre_planes_many_lane<K> (p, t.s[z], y, x)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }

  void pre_mix (const AConvPlan &p, const AConvManyPreTable &t, size_t lanes, int run)
  {
#define PRE(K) for (int z = 0; z < run; z++) for (int y = 0; y < p.out_ch; y++) for (size_t x = 0; x < grid (lanes); x++) aconv_pre_mix_many_lane<K> (p, t.s[z], y, x)
    GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
  }

  /* blockIdx.x = tile, blockIdx.y = stream, 256 lanes, a barrier between the phases */
  void wide_mix (const AConvPlan &p, const AConvWideMatrix &w, const AConvManyPrePlanesTable &t, int in_layout, int tile, size_t tiles, int run)
  {
    std::vector<uint8_t> lds (aconv_wide_lds_bytes (p, tile));
    for (int y = 0; y < run; y++)
      for (size_t bx = 0; bx < tiles; bx++) {
        const AConvManyPrePlanes &m = t.s[y];
        size_t n0;
        int nf;
        if (!aconv_wide_many_tile (m, bx, tile, &n0, &nf))
          continue;
        std::fill (lds.begin (), lds.end (), (uint8_t) 0xcd);                   /* a workgroup finds LDS as whoever ran before left it */
        uint8_t *x = lds.data (), *mat = lds.data () + aconv_wide_x_bytes (p, tile);
        for (int tid = 0; tid < 256; tid++) {
          if (p.mix)
            aconv_wide_stage_matrix (p, w, mat, tid, 256);
#define PRE(K) aconv_wide_stage_lane<K> (p, aconv_many_side (m.in, akind_bytes (K)), in_layout, n0, nf, x, tid, 256)
          GSTAMD_ACONV_FOR_KIND (p.in_kind, PRE);
#undef PRE
        }
        for (int tid = 0; tid < 256; tid++)
          aconv_wide_mix_lane (p, x, mat, w.use, m.mid, n0, nf, tid, 256);
      }
  }

  void post (const AConvPlan &p, const AConvJump *jump, const AConvManyPostTable &t, size_t lanes, int run)
  {
#define POST(K) for (int y = 0; y < run; y++) for (size_t x = 0; x < grid (lanes); x++) aconv_post_many_lane<K> (p, *jump, t.s[y], x)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
  }

  void post_planes (const AConvPlan &p, const AConvJump *jump, const AConvManyPostPlanesTable &t, size_t lanes, int run)
  {
#define POST(K) for (int z = 0; z < run; z++) for (int y = 0; y < p.out_ch; y++) for (size_t x = 0; x < grid (lanes); x++) \
    aconv_post_planes_many_lane<K> (p, *jump, t.s[z], y, x)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, POST);
#undef POST
  }

  void shape (const AConvPlan &p, const AConvManyShapeTable &sh, int run)       /* blockIdx.x = stream, 64 lanes */
  {
#define SHAPE(K) for (int y = 0; y < run; y++) for (int c = 0; c < 64; c++) aconv_shape_many_lane<K> (p, sh.s[y], c)
    GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
  }

  void shape_planes (const AConvPlan &p, const AConvManyShapeTable &sh)         /* one workgroup, lane = stream */
  {
#define SHAPE(K) for (int lane = 0; lane < 64; lane++) aconv_shape_planes_many_lane<K> (p, sh.s[lane])
    GSTAMD_ACONV_FOR_KIND (p.out_kind, SHAPE);
#undef SHAPE
  }

  /* gstamd_audio_resampler_resample_many: independent streams, whatever the launch */
  int resample_many (int run, const AConvManyConv *cs, const AConvManyBuffers *b, const size_t *in_frames, const size_t *out_frames)
  {
    for (int k = 0; k < run; k++)
      emu_audio_resample (cs[k].resampler, b[k].mid_a, in_frames[k], b[k].mid_b, out_frames[k]);
    return GSTAMD_OK;
  }

  /* the run's last launch is over: its buffers go, as device scratch would be free for the next run */
  int launched ()
  {
    pool.clear ();
    return GSTAMD_OK;
  }
};

}  // namespace

extern "C" {

// gstamd_audio_converter_samples_many over emulator handles.  Returns GSTAMD_OK or GSTAMD_ERR_INVALID, as the C ABI does.
int emu_aconv_many_samples (int n, void *const *handles, const int *kind, const void *const *in, const size_t *in_frames, void *const *out, const size_t *out_frames)
{
  EmuManyBackend be = { handles, kind, {} };
  return aconv_many_samples (be, n, in, in_frames, out, out_frames, many_debug);
}

int emu_aconv_many_debug (int32_t *out, int max_out)
{
  for (int i = 0; out && i < 4 && i < max_out; i++)
    out[i] = many_debug[i];
  return 4;
}

// aconv_many_run_length over the same handles, for a test that states the runs: the length of the run that starts at stream 0
int emu_aconv_many_run_length (int n, void *const *handles, const int *kind, const void *const *in, const size_t *in_frames, const size_t *out_frames)
{
  const EmuManyBackend be = { handles, kind, {} };
  std::vector<AConvManyItem> items;
  for (int i = 0; i < n; i++)
    items.push_back (aconv_many_item (be.conv (i), in && in[i] != nullptr, in_frames[i], out_frames[i]));
  return aconv_many_run_length (items.data (), n);
}

}  // extern "C"
