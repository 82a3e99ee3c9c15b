"""Many audio converters in one set of launches: gstamd_audio_converter_samples_many.

Nothing here needs the reference tree.  The expected bytes of every case are those of FRESH converters made with the same arguments and driven by
gstamd_audio_converter_samples, one call per stream per round, in array order - the entry tests/test_audio_convert.py pins against the reference.
The debug counters of the call (batched runs, streams served by them, streams gone one by one, launches of the batched kernels) are checked with
the bytes, so a loop of single calls behind the new name fails too.

A. equal plans, streams of unequal length whose buffers start 0 .. 3 samples into their allocations, three rounds (dither position, tpdf-hf's
   previous draw and the error history carry);  B. the resampler inside, a stream that yields no output inside a batch, a drain round;
C. a mixed array: two plans alternating, a wide converter, a non-interleaved output, a passthrough, an endian plan;  D. the same converter twice;
E. more than 64 streams;  F. n = 0, an empty stream inside a run, the refusals;  G. emulator and device agree byte for byte (GPU only).

Every check runs twice: -m "not gpu" through the kernel bodies on the host emulator (tests/emu/emu_audio_many.cpp: the library's own walk of the
call, aconv_many_samples of audio_convert_plan.h, over a backend that loops over the grid of each batched launch), -m gpu through the C ABI on the
device.  There is one run rule (aconv_many_run_length) and one emulator of it; tests/test_audio_convert_many_layouts.py uses the same one.  Output
blocks sit between guard bytes that must survive."""
import ctypes as C

import numpy as np
import pytest

from gstreamer_amd import audio as A
import test_audio_convert_layouts as L
import test_audio_convert_wide as W

BYTES = A.AFMT_BYTES
GUARD = L.GUARD
SURROUND = L.SURROUND
ERR_INVALID = -1                # GSTAMD_ERR_INVALID (include/gstamd_video.h); checked against the binding in the GPU tests


class Plan:
    """the arguments of one converter"""

    def __init__(self, ifmt, ofmt, in_ch=2, out_ch=None, in_rate=48000, out_rate=None, il=0, ol=0, wide=False, in_pos=None, out_pos=None, **cfg):
        self.ifmt, self.ofmt, self.in_ch, self.out_ch = ifmt, ofmt, in_ch, in_ch if out_ch is None else out_ch
        self.in_rate, self.out_rate, self.il, self.ol, self.wide, self.in_pos, self.out_pos, self.cfg = in_rate, out_rate or in_rate, il, ol, wide, in_pos, out_pos, cfg

    def infos(self):
        mk = A.audio_info_wide if self.wide else A.audio_info
        return mk(self.ifmt, self.in_rate, self.in_ch, self.in_pos), mk(self.ofmt, self.out_rate, self.out_ch, self.out_pos)

    @property
    def kind(self):
        """emu_aconv_many_samples' kind[]: 0 a handle of emu_aconv_planes_new, 1 of emu_aconv_wide_new, 3 the latter with a resampler"""
        return 0 if not self.wide else 3 if self.in_rate != self.out_rate else 1

    @property
    def shapes(self):
        return self.cfg.get("noise_shaping", "none") != "none"


# ---- backends ------------------------------------------------------------------------------------------------------------------------
class EmuMany:
    """tests/emu/emu_audio_many.cpp over the handles of emu_audio_planes.cpp / emu_audio_wide.cpp"""

    def __init__(self, emu):
        self.emu, self.planes, self.wide = emu, L.EmuBackend(emu), W.EmuWide(emu)
        pp, ps = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        emu.emu_aconv_many_samples.argtypes = [C.c_int, pp, C.POINTER(C.c_int), pp, ps, pp, ps]
        emu.emu_aconv_many_debug.argtypes = [C.POINTER(C.c_int32), C.c_int]
        emu.emu_aconv_many_run_length.argtypes = [C.c_int, pp, C.POINTER(C.c_int), pp, ps, ps]

    def new(self, plan):
        ii, oi = plan.infos()
        cfg = A.audio_converter_config(**plan.cfg)
        return (self.wide.new(ii, plan.il, oi, plan.ol, cfg) if plan.wide else self.planes.new(ii, plan.il, oi, plan.ol, cfg)), plan.kind

    def free(self, c):
        (self.wide if c[1] else self.planes).free(c[0])

    def out_frames(self, c, n):
        return (self.wide if c[1] else self.planes).out_frames(c[0], n)

    def upload(self, host):
        a = np.zeros(host.size + 16, np.uint8)
        o = (-a.ctypes.data) % 16
        a[o: o + host.size] = host
        return (a, o, host.size), a.ctypes.data + o

    def download(self, keep):
        a, o, n = keep
        return a[o: o + n].copy()

    def single(self, c, src, n, dst, on):
        (self.wide if c[1] else self.planes).f("samples")(c[0], src, n, dst, on)
        return 0

    @staticmethod
    def _arrays(convs, srcs, in_frames, dsts, out_frames):
        n = len(in_frames)
        hs = None if convs is None else (C.c_void_p * n)(*[None if c is None else c[0] for c in convs])
        kinds = None if convs is None else (C.c_int * n)(*[0 if c is None else c[1] for c in convs])
        ip = None if srcs is None else (C.c_void_p * n)(*srcs)
        return n, hs, kinds, ip, (C.c_size_t * n)(*in_frames), (C.c_void_p * n)(*dsts), (C.c_size_t * n)(*out_frames)

    def many(self, convs, srcs, in_frames, dsts, out_frames):
        return self.emu.emu_aconv_many_samples(*self._arrays(convs, srcs, in_frames, dsts, out_frames))

    def run_length(self, convs, srcs, in_frames, out_frames):
        """aconv_many_run_length itself: the run that starts at the first of these streams"""
        n, hs, kinds, ip, inf, _, outf = self._arrays(convs, srcs, in_frames, [None] * len(convs), out_frames)
        return self.emu.emu_aconv_many_run_length(n, hs, kinds, ip, inf, outf)

    def debug(self):
        buf = (C.c_int32 * 4)()
        assert self.emu.emu_aconv_many_debug(buf, 4) == 4
        return list(buf)


class GpuMany:
    """the HIP path through the C ABI (gstreamer_amd.audio.ManyConversions)"""

    def __init__(self, dev):
        self.dev = dev

    def new(self, plan):
        ii, oi = plan.infos()
        cfg = A.audio_converter_config(**plan.cfg)
        if plan.wide:
            return A.AudioConverterWide(ii, oi, cfg, in_layout=plan.il, out_layout=plan.ol)
        return A.AudioConverter(ii, oi, cfg, in_layout=plan.il, out_layout=plan.ol) if plan.il or plan.ol else A.AudioConverter(ii, oi, cfg)

    def free(self, c):
        c.free()

    def out_frames(self, c, n):
        return c.get_out_frames(n)

    def upload(self, host):
        import torch
        t = torch.zeros(host.size + 16, dtype=torch.uint8, device=self.dev)
        o = (-t.data_ptr()) % 16
        t[o: o + host.size] = torch.from_numpy(host).to(self.dev)
        return (t, o, host.size), t.data_ptr() + o

    def download(self, keep):
        import torch
        t, o, n = keep
        torch.cuda.synchronize()
        return t.cpu().numpy()[o: o + n].copy()

    def single(self, c, src, n, dst, on):
        return A._conv_lib().gstamd_audio_converter_samples(c._h, 0, src, n, dst, on, None)

    def many(self, convs, srcs, in_frames, dsts, out_frames):
        n = len(in_frames)
        if convs is None:                       # a NULL `converters` array
            ip = (C.c_void_p * n)(*srcs)
            return A._conv_lib().gstamd_audio_converter_samples_many(n, None, 0, ip, (C.c_size_t * n)(*in_frames), (C.c_void_p * n)(*dsts),
                                                                     (C.c_size_t * n)(*out_frames), None)
        from gstreamer_amd import video as V
        try:
            A.convert_many(convs, srcs, in_frames, dsts, out_frames)
        except V.GstAmdError as e:
            assert str(e)
            return e.code
        return 0

    def debug(self):
        d = A.convert_many_debug()
        return [d["runs"], d["batched"], d["single"], d["launches"]]


@pytest.fixture
def emu_backend(native_lib, emu_lib):
    return EmuMany(emu_lib)


@pytest.fixture
def gpu_backend(native_lib, gpu):
    from gstreamer_amd import video as V
    assert V.ERR_INVALID == ERR_INVALID
    return GpuMany(gpu)


# ---- one call's buffers: every stream's input and output block inside one allocation, between guard bytes -------------------------------
class Bufs:
    """blocks[k] = (bytes or None, offset): block k starts `offset` bytes past a 16-byte boundary, 32 guard bytes (and the offset) in front of it, 32
    or more behind it; a block given as a size is filled with the guard pattern (an output)"""

    def __init__(self, be, blocks):
        self.be, self.offs, self.sizes, pos = be, [], [], 0
        for data, off in blocks:
            size = data if isinstance(data, int) else data.size
            self.offs.append(pos + 32 + off)
            self.sizes.append(size)
            pos += (32 + off + size + 32 + 15) // 16 * 16
        host = np.full(pos, GUARD, np.uint8)
        for (data, _), o, s in zip(blocks, self.offs, self.sizes):
            if not isinstance(data, int):
                host[o: o + s] = data
        self.keep, self.base = be.upload(host)

    def ptr(self, k):
        return self.base + self.offs[k]

    def read(self):
        """the blocks; nothing outside them was written"""
        got = self.be.download(self.keep)
        L.check_guards(got, self.offs, self.sizes)
        return [got[o: o + s].copy() for o, s in zip(self.offs, self.sizes)]


def call(be, plans, convs, streams, mode):
    """one call over streams = [(raw bytes or None, in_frames, out_frames, input offset, output offset in samples)]: `many`, or one single call per
    stream in array order.  Returns the output blocks and - for `many` - the debug counters."""
    ins = Bufs(be, [(np.zeros(0, np.uint8) if raw is None else raw, io * BYTES[p.ifmt]) for p, (raw, _, _, io, _) in zip(plans, streams)])
    outs = Bufs(be, [(on * p.out_ch * BYTES[p.ofmt], oo * BYTES[p.ofmt]) for p, (_, _, on, _, oo) in zip(plans, streams)])
    srcs = [None if s[0] is None else ins.ptr(k) for k, s in enumerate(streams)]
    dsts = [outs.ptr(k) for k in range(len(streams))]
    counters = None
    if mode == "many":
        assert be.many(convs, srcs, [s[1] for s in streams], dsts, [s[2] for s in streams]) == 0
        counters = be.debug()
    else:
        for c, s, src, dst in zip(convs, streams, srcs, dsts):
            assert be.single(c, src, s[1], dst, s[2]) == 0
    return outs.read(), counters


def drive(be, plans, rounds, modes, share=None):
    """fresh converters for `plans` (share[k]: the index of the converter stream k uses, for the same converter twice); rounds[r][k] = (raw or None,
    in_frames, input offset, output offset); out_frames come from get_out_frames before each call, as a caller gets them.  Returns, per round, the
    output blocks, the counters and what get_out_frames answers afterwards."""
    share = list(range(len(plans))) if share is None else share
    made = {}
    for k, j in enumerate(share):
        if j not in made:
            made[j] = be.new(plans[k])
    convs = [made[j] for j in share]
    try:
        res = []
        for rnd, mode in zip(rounds, modes):
            # (the same converter twice in a call: its second out_frames is asked for before its first buffer went in - without a resampler it is in_frames)
            streams = [(raw, n, be.out_frames(c, n), io, oo) for c, (raw, n, io, oo) in zip(convs, rnd)]
            blocks, counters = call(be, plans, convs, streams, mode)
            res.append((blocks, counters, [be.out_frames(c, 1000) for c in convs]))
        return res
    finally:
        for c in made.values():
            be.free(c)


def check_equal(got, exp, what):
    assert len(got) == len(exp)
    for r, ((gb, _, gf), (eb, _, ef)) in enumerate(zip(got, exp)):
        L.same(gb, eb, (what, "round", r))
        assert gf == ef, (what, "get_out_frames after round", r)


def make_rounds(plans, frames, n_rounds, seed, offsets=True):
    return [[(L.stream(p.ifmt, p.in_ch, n, seed + 97 * r + 7 * k), n, (k + r) % 4 if offsets else 0, (3 * k + r + 1) % 4 if offsets else 0)
             for k, (p, n) in enumerate(zip(plans, frames))] for r in range(n_rounds)]


# ---- A. equal plans, unequal streams ------------------------------------------------------------------------------------------------
A_FRAMES = (1, 5, 67, 333, 1024, 1027, 4)
A_PLANS = {
    "f32_s16_tpdf_high": Plan("F32LE", "S16LE", dither_method="tpdf", noise_shaping="high"),
    "s32_s24be": Plan("S32LE", "S24BE", dither_method="none", noise_shaping="none"),
    "f64_u8_mono_rpdf_feedback": Plan("F64LE", "U8", in_ch=1, dither_method="rpdf", noise_shaping="error-feedback"),
    "f32_s16_tpdfhf_medium": Plan("F32LE", "S16LE", dither_method="tpdf-hf", noise_shaping="medium"),
    "s16_f32": Plan("S16LE", "F32LE"),
    "f32_51_s16_stereo_tpdf": Plan("F32LE", "S16LE", in_ch=6, out_ch=2, in_pos=SURROUND, dither_method="tpdf"),
    "s16_stereo_s16_mono": Plan("S16LE", "S16LE", in_ch=2, out_ch=1),
}


def case_a(be, name, modes=("many",) * 3):
    plan = A_PLANS[name]
    plans = [plan] * len(A_FRAMES)
    return plans, drive(be, plans, make_rounds(plans, A_FRAMES, 3, 11 + len(name)), modes)


def check_equal_plans(be, name):
    plans, got = case_a(be, name)
    _, exp = case_a(be, name, ("single",) * 3)
    check_equal(got, exp, name)
    assert sum(b.size for b in exp[0][0]) > 0
    for _, counters, _ in got:                  # one batched run of 7, nothing one by one; first and second kernel, and the shaping kernel of a plan that has one
        assert counters == [1, 7, 0, 3 if plans[0].shapes else 2], (name, counters)


@pytest.mark.parametrize("name", sorted(A_PLANS))
def test_equal_plans_unequal_streams_on_host(emu_backend, name):
    check_equal_plans(emu_backend, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(A_PLANS))
def test_equal_plans_unequal_streams_on_device(gpu_backend, name):
    check_equal_plans(gpu_backend, name)


# ---- B. the resampler inside --------------------------------------------------------------------------------------------------------
B_FRAMES = (1, 64, 300, 1024, 1000)
B_PLAN = Plan("F32LE", "S16LE", in_rate=48000, out_rate=44100, dither_method="tpdf", noise_shaping="medium")
B_MODES = ("many",) * 4


def case_b(be, modes=B_MODES):
    plans = [B_PLAN] * len(B_FRAMES)
    rounds = make_rounds(plans, B_FRAMES, 3, 5)
    rounds.append([(None, 32, 0, (k + 1) % 4) for k in range(len(plans))])              # the drain: silence into every resampler
    return drive(be, plans, rounds, modes)


def check_resampler_inside(be):
    got, exp = case_b(be), case_b(be, ("single",) * 4)
    check_equal(got, exp, "resampler")
    assert exp[0][0][0].size == 0 and exp[0][0][1].size > 0, "the first round's 1-frame stream yields no output, inside a batch"
    assert all(b.size > 0 for b in exp[3][0]), "the drain round brings out what the filters hold"
    assert [c for _, c, _ in got] == [[1, 5, 0, 3]] * 3 + [[0, 0, 5, 0]], "three batched rounds; a NULL input goes one by one"


def test_resampler_inside_on_host(emu_backend):
    check_resampler_inside(emu_backend)


@pytest.mark.gpu
def test_resampler_inside_on_device(gpu_backend):
    check_resampler_inside(gpu_backend)


# ---- C. a mixed array -----------------------------------------------------------------------------------------------------------------
def case_c():
    p = Plan("F32LE", "S16LE", dither_method="tpdf")
    q = Plan("S32LE", "S24LE", dither_method="none")
    wide = Plan("F32LE", "S16LE", in_ch=12, wide=True, dither_method="rpdf")
    planar = Plan("F32LE", "S16LE", ol=1, dither_method="tpdf")
    passthrough = Plan("S16LE", "S16LE")
    endian = Plan("S16LE", "S16BE")
    plans = [p, q, p, p, q, q, wide, planar, passthrough, endian]
    frames = (67, 5, 333, 64, 100, 9, 33, 40, 17, 21)
    # aconv_many_run_length from each stream on: P | Q | P P | Q Q | and the four that never batch
    runs = (1, 1, 2, 1, 2, 1, 1, 1, 1, 1)
    return plans, frames, runs


def check_mixed_array(be):
    plans, frames, _ = case_c()
    rounds = make_rounds(plans, frames, 2, 3)
    got, exp = drive(be, plans, rounds, ("many",) * 2), drive(be, plans, rounds, ("single",) * 2)
    check_equal(got, exp, "mixed")
    # P P and Q Q are the batched runs (two launches each: neither plan shapes); P, Q and the other four go one by one
    assert [c for _, c, _ in got] == [[2, 4, 6, 4]] * 2


def test_mixed_array_on_host(emu_backend):
    check_mixed_array(emu_backend)


@pytest.mark.gpu
def test_mixed_array_on_device(gpu_backend):
    check_mixed_array(gpu_backend)


def test_run_lengths_of_the_mixed_array(emu_backend):
    """aconv_many_run_length (audio_convert_plan.h), which the library and the emulator both walk the array with"""
    be = emu_backend
    plans, frames, runs = case_c()
    convs = [be.new(p) for p in plans]
    try:
        src = [1] * len(plans)                  # any non-NULL input: the decision takes no device pointers
        for k, exp in enumerate(runs):
            assert be.run_length(convs[k:], src[k:], frames[k:], frames[k:]) == exp, k
        pp = [convs[2], convs[3]]
        assert be.run_length(pp, [1, 1], [8, 8], [8, 8]) == 2
        assert be.run_length(pp, [1, None], [8, 8], [8, 8]) == 1, "a NULL input does not join a run"
        assert be.run_length(pp, [None, 1], [8, 8], [8, 8]) == 1, "... and does not start one"
        assert be.run_length(pp, [1, 1], [8, 1 << 30], [8, 1 << 30]) == 1, "2^30 frames do not join a run"
        assert be.run_length(pp, [1, 1], [(1 << 30) - 1, 8], [(1 << 30) - 1, 8]) == 2
        assert be.run_length([convs[2], convs[3], convs[2]], [1] * 3, [8] * 3, [8] * 3) == 2, "the same converter twice ends the run"
        many = [be.new(plans[0]) for _ in range(70)]
        assert be.run_length(many, [1] * 70, [8] * 70, [8] * 70) == 64
        for c in many:
            be.free(c)
        # a resampler inside is part of what a run shares
        r = be.new(Plan("F32LE", "S16LE", in_rate=48000, out_rate=44100, dither_method="tpdf"))
        assert be.run_length([convs[0], r], [1, 1], [8, 8], [8, 7]) == 1
        be.free(r)
    finally:
        for c in convs:
            be.free(c)


# ---- D. the same converter twice ------------------------------------------------------------------------------------------------------
def check_duplicates(be):
    plan = Plan("F32LE", "S16LE", dither_method="tpdf", noise_shaping="high")
    plans, share = [plan] * 3, [0, 1, 0]
    rounds = make_rounds(plans, (67, 40, 33), 2, 9)
    # round 0: [c0, c1, c0] in one call; round 1: single calls on both sides - c0's state is that of two calls
    got, exp = drive(be, plans, rounds, ("many", "single"), share), drive(be, plans, rounds, ("single", "single"), share)
    check_equal(got, exp, "duplicates")
    assert got[0][1] == [1, 2, 1, 3], "c0 c1 share the launches, c0's second buffer follows by itself"


def test_duplicates_on_host(emu_backend):
    check_duplicates(emu_backend)


@pytest.mark.gpu
def test_duplicates_on_device(gpu_backend):
    check_duplicates(gpu_backend)


# ---- E. more than 64 ---------------------------------------------------------------------------------------------------------------------
def check_more_than_64(be):
    plans = [Plan("S32LE", "S16LE", in_ch=1, dither_method="rpdf")] * 70
    rounds = make_rounds(plans, (33,) * 70, 1, 21)
    got, exp = drive(be, plans, rounds, ("many",)), drive(be, plans, rounds, ("single",))
    check_equal(got, exp, "70 streams")
    assert got[0][1] == [2, 70, 0, 4], "64 + 6"


def test_more_than_64_on_host(emu_backend):
    check_more_than_64(emu_backend)


@pytest.mark.gpu
def test_more_than_64_on_device(gpu_backend):
    check_more_than_64(gpu_backend)


# ---- F. edges -------------------------------------------------------------------------------------------------------------------------
F_PLAN = Plan("F32LE", "S16LE", dither_method="tpdf")
F_FRAMES = 33


def first_call_bytes(be, raw):
    c = be.new(F_PLAN)
    try:
        blocks, _ = call(be, [F_PLAN], [c], [(raw, F_FRAMES, F_FRAMES, 0, 0)], "single")
        return blocks[0]
    finally:
        be.free(c)


def check_untouched(be, convs, raws, outs, skip=()):
    """the outputs still hold the guard pattern, and every converter's next single call gives a first call's bytes: its state did not move"""
    for k, b in enumerate(outs.read()):
        assert k in skip or (b == GUARD).all(), k
    for k, c in enumerate(convs):
        if k not in skip:
            blocks, _ = call(be, [F_PLAN], [c], [(raws[k], F_FRAMES, F_FRAMES, 0, 0)], "single")
            L.same([blocks[0]], [first_call_bytes(be, raws[k])], ("a first call", k))


def check_edges(be):
    assert be.many([], [], [], [], []) == 0 and be.debug() == [0, 0, 0, 0], "n = 0"
    raws = [L.stream("F32LE", 2, F_FRAMES, 40 + k) for k in range(3)]
    size = F_FRAMES * 2 * 2

    def setup():
        convs = [be.new(F_PLAN) for _ in range(3)]
        ins, outs = Bufs(be, [(r, 0) for r in raws]), Bufs(be, [(size, 0)] * 3)
        return convs, ins, outs, [ins.ptr(k) for k in range(3)], [outs.ptr(k) for k in range(3)]

    # an empty stream inside a run: skipped, the two around it share their launches
    convs, ins, outs, srcs, dsts = setup()
    assert be.many(convs, srcs, [F_FRAMES, 0, F_FRAMES], dsts, [F_FRAMES, F_FRAMES, F_FRAMES]) == 0
    assert be.debug() == [1, 2, 0, 2]
    blocks = outs.read()
    L.same([blocks[0], blocks[2]], [first_call_bytes(be, raws[0]), first_call_bytes(be, raws[2])], "around the empty stream")
    check_untouched(be, convs, raws, outs, skip=(0, 2))
    for c in convs:
        be.free(c)

    # refusals: GSTAMD_ERR_INVALID before anything is launched
    n3 = [F_FRAMES] * 3
    for what, args in (("NULL converters", lambda cv, s, d: (None, s, n3, d, n3)),
                       ("a NULL converter", lambda cv, s, d: ([cv[0], None, cv[2]], s, n3, d, n3)),
                       ("a NULL out[i]", lambda cv, s, d: (cv, s, n3, [d[0], d[1], None], n3)),
                       ("in_frames != out_frames without a resampler", lambda cv, s, d: (cv, s, n3, d, [F_FRAMES, F_FRAMES, F_FRAMES - 1])),
                       ("a NULL input without a resampler", lambda cv, s, d: (cv, [s[0], s[1], None], n3, d, n3))):
        convs, ins, outs, srcs, dsts = setup()
        assert be.many(*args(convs, srcs, dsts)) == ERR_INVALID, what
        assert be.debug() == [0, 0, 0, 0], what
        check_untouched(be, convs, raws, outs)
        for c in convs:
            be.free(c)


def test_edges_on_host(emu_backend):
    check_edges(emu_backend)


@pytest.mark.gpu
def test_edges_on_device(gpu_backend):
    check_edges(gpu_backend)


# ---- G. emulator and device agree -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_emulator_and_device_agree(gpu_backend, emu_lib):
    emu = EmuMany(emu_lib)
    _, on_host = case_a(emu, "f32_s16_tpdfhf_medium")
    _, on_device = case_a(gpu_backend, "f32_s16_tpdfhf_medium")
    check_equal(on_device, on_host, "tpdf-hf + medium")
    assert [c for _, c, _ in on_device] == [c for _, c, _ in on_host]
    on_host, on_device = case_b(emu), case_b(gpu_backend)
    check_equal(on_device, on_host, "resampler")
    assert [c for _, c, _ in on_device] == [c for _, c, _ in on_host]
