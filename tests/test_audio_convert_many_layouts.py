"""Non-interleaved and wide converters in the batched runs of gstamd_audio_converter_samples_many.

Nothing here needs the reference tree.  As in tests/test_audio_convert_many.py, whose helpers this file uses, the expected bytes of every case are
those of FRESH converters made with the same arguments and driven by gstamd_audio_converter_samples, one call per stream per round, in array order:
output bytes, the next rounds' bytes (dither position, shaping history, resampler history) and get_out_frames.  Every case asserts the call's debug
counters - batched runs, streams they served, streams gone one by one, launches of the batched kernels - so a library that sends a planar or a
wide stream through the single path fails each of them.

A. planar in, interleaved out;  B. interleaved in, planar out;  C. planar to planar;  D. the resampler inside, a stream without output, a drain
round;  E. wide converters, two of which differ in the mix matrix only;  F. the run rules with the run lengths stated;  G. the refusals;
H. emulator and device agree byte for byte (GPU only).

A non-interleaved side is one block, plane after plane (what gstamd_audio_converter_samples takes); blocks start 0 .. 3 samples into their
allocations and sit between guard bytes that must survive.  Every check runs twice: -m "not gpu" through the kernel bodies on the host emulator
(tests/emu/emu_audio_many.cpp, the one emulator of the call: the library's own walk, aconv_many_samples of audio_convert_plan.h, over a backend
that loops over the grid of each batched launch), -m gpu through the C ABI on the device."""
import numpy as np
import pytest

from gstreamer_amd import audio as A
import test_audio_convert_layouts as L
import test_audio_convert_many as M

GUARD = L.GUARD
SURROUND = L.SURROUND
ERR_INVALID = M.ERR_INVALID
BYTES = A.AFMT_BYTES


class Plan(M.Plan):
    """M.Plan with the mix_matrix argument of a wide converter ([out][in] rows)"""

    def __init__(self, *a, matrix=None, **kw):
        M.Plan.__init__(self, *a, **kw)
        self.matrix = matrix


class EmuMany(M.EmuMany):
    """M.EmuMany (tests/emu/emu_audio_many.cpp) with the mix matrix of a wide converter"""

    def new(self, plan):
        if not plan.wide:
            return M.EmuMany.new(self, plan)
        ii, oi = plan.infos()
        return self.wide.new(ii, plan.il, oi, plan.ol, A.audio_converter_config(**plan.cfg), plan.matrix), plan.kind


class GpuMany(M.GpuMany):
    def new(self, plan):
        if not plan.wide:
            return M.GpuMany.new(self, plan)
        ii, oi = plan.infos()
        return A.AudioConverterWide(ii, oi, A.audio_converter_config(**plan.cfg), in_layout=plan.il, out_layout=plan.ol, mix_matrix=plan.matrix)


@pytest.fixture
def emu_backend(native_lib, emu_lib):
    return EmuMany(emu_lib)


@pytest.fixture
def gpu_backend(native_lib, gpu):
    from gstreamer_amd import video as V
    assert V.ERR_INVALID == ERR_INVALID
    return GpuMany(gpu)


def rounds_of(plans, frames_of_round, seed):
    """frames_of_round[r][k]: the frames of stream k in round r; the blocks start (k + r) % 4 and (3 k + r + 1) % 4 samples into their allocations"""
    return [[(L.stream(p.ifmt, p.in_ch, n, seed + 97 * r + 7 * k), n, (k + r) % 4, (3 * k + r + 1) % 4) for k, (p, n) in enumerate(zip(plans, frames))]
            for r, frames in enumerate(frames_of_round)]


def both(be, plans, rounds, modes=None, share=None):
    """the call under test and the fresh converters driven one by one; returns what the batched side did"""
    modes = modes or ("many",) * len(rounds)
    got, exp = M.drive(be, plans, rounds, modes, share), M.drive(be, plans, rounds, ("single",) * len(rounds), share)
    M.check_equal(got, exp, "many against single calls")
    return got, exp


def launches(plan):
    return 3 if plan.shapes else 2


# ---- A / B / C: seven streams of one plan, three rounds -----------------------------------------------------------------------------------
# 11 and 13 frames are the two sides of the realign condition (frames >= 12) of planes on different byte phases, 3 and 4 those of the first
# four-frame lane, 1027 takes more than one block of a plane; every round gives a stream another count, so all eight are used
FRAME_SET = (1, 3, 4, 11, 12, 13, 67, 1027)
STREAMS = 7

PLANS = {
    # A. planar in, interleaved out
    "a_f32p_s16_tpdf_high": Plan("F32LE", "S16LE", il=1, dither_method="tpdf", noise_shaping="high"),
    "a_s24p_3ch_f32": Plan("S24LE", "F32LE", in_ch=3, il=1),
    "a_s16p_s16": Plan("S16LE", "S16LE", il=1),
    "a_u8p_mono_s16": Plan("U8", "S16LE", in_ch=1, il=1),
    # B. interleaved in, planar out
    "b_f32_s16p_tpdfhf_medium": Plan("F32LE", "S16LE", ol=1, dither_method="tpdf-hf", noise_shaping="medium"),
    "b_s32_s24p": Plan("S32LE", "S24LE", ol=1, dither_method="none"),
    "b_f32_8ch_s16p_tpdf": Plan("F32LE", "S16LE", in_ch=8, ol=1, dither_method="tpdf"),
    # C. planar to planar: rows are planes; the 5.1 down-mix
    "c_f32p_s16p_rpdf_feedback": Plan("F32LE", "S16LE", il=1, ol=1, dither_method="rpdf", noise_shaping="error-feedback"),
    "c_s24p_51_s16p_stereo": Plan("S24LE", "S16LE", in_ch=6, out_ch=2, il=1, ol=1, in_pos=SURROUND, dither_method="tpdf"),
    "c_f32p_51_f32p_stereo": Plan("F32LE", "F32LE", in_ch=6, out_ch=2, il=1, ol=1, in_pos=SURROUND),
}


def case_abc(be, name, modes=("many",) * 3):
    plan = PLANS[name]
    plans = [plan] * STREAMS
    frames = [[FRAME_SET[(k + 3 * r) % len(FRAME_SET)] for k in range(STREAMS)] for r in range(3)]
    return plans, M.drive(be, plans, rounds_of(plans, frames, 31 + len(name)), modes)


def check_one_plan(be, name):
    plans, got = case_abc(be, name)
    _, exp = case_abc(be, name, ("single",) * 3)
    M.check_equal(got, exp, name)
    assert sum(b.size for b in exp[0][0]) > 0
    for _, counters, _ in got:                  # one batched run of seven, nothing one by one
        assert counters == [1, STREAMS, 0, launches(plans[0])], (name, counters)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_one_plan_seven_streams_on_host(emu_backend, name):
    check_one_plan(emu_backend, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PLANS))
def test_one_plan_seven_streams_on_device(gpu_backend, name):
    check_one_plan(gpu_backend, name)


# ---- D. the resampler inside ------------------------------------------------------------------------------------------------------------
D_FRAMES = (1, 64, 300, 257, 13)
D_PLAN = Plan("F32LE", "S16LE", in_rate=48000, out_rate=44100, il=1, ol=1, dither_method="tpdf", noise_shaping="medium")


def case_d(be, modes=("many",) * 4):
    plans = [D_PLAN] * len(D_FRAMES)
    rounds = rounds_of(plans, [D_FRAMES] * 3, 5)
    rounds.append([(None, 32, 0, (k + 1) % 4) for k in range(len(plans))])              # the drain: silence into every resampler
    return M.drive(be, plans, rounds, modes)


def check_resampler_inside(be):
    got, exp = case_d(be), case_d(be, ("single",) * 4)
    M.check_equal(got, exp, "resampler")
    assert exp[0][0][0].size == 0 and exp[0][0][1].size > 0, "the first round's 1-frame stream yields no output, inside a batch"
    assert all(b.size > 0 for b in exp[3][0]), "the drain round brings out what the filters hold"
    assert [c for _, c, _ in got] == [[1, 5, 0, 3]] * 3 + [[0, 0, 5, 0]], "three batched rounds; a NULL input goes one by one"


def test_resampler_inside_on_host(emu_backend):
    check_resampler_inside(emu_backend)


@pytest.mark.gpu
def test_resampler_inside_on_device(gpu_backend):
    check_resampler_inside(gpu_backend)


# ---- E. wide converters -------------------------------------------------------------------------------------------------------------------
def matrix(out_ch, in_ch, seed):
    rng = np.random.RandomState(seed)
    m = rng.uniform(0.05, 0.9, (out_ch, in_ch)) * rng.choice([-1.0, 1.0], (out_ch, in_ch)) / np.sqrt(in_ch)
    return [[float(np.float32(v)) for v in row] for row in m]


E_PLANS = {
    # both sides interleaved, no mix: the kernels of the ordinary plan on 12 channels
    "e_12ch_f32_s16_rpdf": (Plan("F32LE", "S16LE", in_ch=12, wide=True, dither_method="rpdf"), (33, 5, 171, 1)),
    # 16 planes through the LDS tile kernel (a tile is 128 frames: the third stream has a tile edge inside and two tiles) into 6 planes
    "e_16ch_s24p_6ch_s24p_matrix": (Plan("S24LE", "S24LE", in_ch=16, out_ch=6, il=1, ol=1, wide=True, matrix=matrix(6, 16, 3), dither_method="none"), (11, 13, 131, 4)),
    "e_16ch_s24p_6ch_s16p_matrix_tpdf_high": (Plan("S24LE", "S16LE", in_ch=16, out_ch=6, il=1, ol=1, wide=True, matrix=matrix(6, 16, 4), dither_method="tpdf",
                                                   noise_shaping="high"), (12, 3, 67, 129)),
    "e_64ch_f32p_s16p_tpdfhf_simple": (Plan("F32LE", "S16LE", in_ch=64, il=1, ol=1, wide=True, dither_method="tpdf-hf", noise_shaping="simple"), (33, 1, 12, 35)),
    "e_12ch_f32p_s16_resampler": (Plan("F32LE", "S16LE", in_ch=12, il=1, wide=True, in_rate=48000, out_rate=44100, dither_method="tpdf"), (64, 1, 100, 37)),
}


def case_e(be, name, modes=("many",) * 2):
    plan, frames = E_PLANS[name]
    plans = [plan] * len(frames)
    return plans, M.drive(be, plans, rounds_of(plans, [frames, frames[::-1]], 71 + len(name)), modes)


def check_wide(be, name):
    plans, got = case_e(be, name)
    _, exp = case_e(be, name, ("single",) * 2)
    M.check_equal(got, exp, name)
    assert sum(b.size for b in exp[0][0]) > 0
    for _, counters, _ in got:
        assert counters == [1, len(plans), 0, launches(plans[0])], (name, counters)


@pytest.mark.parametrize("name", sorted(E_PLANS))
def test_wide_converters_on_host(emu_backend, name):
    check_wide(emu_backend, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(E_PLANS))
def test_wide_converters_on_device(gpu_backend, name):
    check_wide(gpu_backend, name)


def check_wide_matrices(be):
    """two wide converters that differ in mix_matrix only have equal AConvPlans: they must not share a run, and each gives its own bytes"""
    kw = dict(in_ch=12, out_ch=4, il=1, ol=1, wide=True, dither_method="rpdf")
    m1, m2 = Plan("F32LE", "S16LE", matrix=matrix(4, 12, 1), **kw), Plan("F32LE", "S16LE", matrix=matrix(4, 12, 2), **kw)
    plans = [m1, m1, m2, m2]
    rounds = rounds_of(plans, [(40,) * 4] * 2, 13)
    rounds = [[(rnd[0][0], n, io, oo) for (_, n, io, oo) in rnd] for rnd in rounds]      # the same samples into all four
    got, exp = both(be, plans, rounds)
    assert [c for _, c, _ in got] == [[2, 4, 0, 4]] * 2
    assert not (exp[0][0][0] == exp[0][0][2]).all(), "the two matrices give different bytes for the same samples"
    plans = [m1, m2, m1]
    got, _ = both(be, plans, [rnd[:3] for rnd in rounds])
    assert [c for _, c, _ in got] == [[0, 0, 3, 0]] * 2


def test_wide_matrices_do_not_share_a_run_on_host(emu_backend):
    check_wide_matrices(emu_backend)


@pytest.mark.gpu
def test_wide_matrices_do_not_share_a_run_on_device(gpu_backend):
    check_wide_matrices(gpu_backend)


# ---- F. the run rules -----------------------------------------------------------------------------------------------------------------------
MONO_P = Plan("F32LE", "S16LE", in_ch=1, il=1, ol=1, dither_method="tpdf")
MONO_I = Plan("F32LE", "S16LE", in_ch=1, dither_method="tpdf")          # the same AConvPlan byte for byte: q_stride is 1 in both
STEREO_I = Plan("F32LE", "S16LE", dither_method="tpdf")
STEREO_OP = Plan("F32LE", "S16LE", ol=1, dither_method="tpdf")
PLANAR = Plan("F32LE", "S16LE", il=1, ol=1, dither_method="tpdf", noise_shaping="high")


def test_run_lengths(emu_backend):
    """aconv_many_run_length (audio_convert_plan.h) as the library calls it, which the library and the emulator both walk the array with"""
    be = emu_backend
    plans = dict(mp=MONO_P, mi=MONO_I, si=STEREO_I, sop=STEREO_OP, pl=PLANAR, pt=Plan("S16LE", "S16LE", il=1, ol=1), en=Plan("S16LE", "S16BE", il=1, ol=1),
                 w=E_PLANS["e_64ch_f32p_s16p_tpdfhf_simple"][0], wpt=Plan("S16LE", "S16LE", in_ch=12, il=1, ol=1, wide=True))
    c = {k: [be.new(p) for _ in range(3)] for k, p in plans.items()}
    try:
        def run(*convs, src=None, frames=None):
            n = len(convs)
            return be.run_length(list(convs), src or [1] * n, frames or [8] * n, frames or [8] * n)

        assert run(*c["mp"]) == 3 and run(*c["mi"]) == 3 and run(*c["pl"]) == 3 and run(*c["w"]) == 3
        assert run(c["mp"][0], c["mi"][0]) == 1 and run(c["mi"][0], c["mp"][0]) == 1, "equal plan bytes, different layouts"
        assert run(c["mp"][0], c["mp"][1], c["mi"][0], c["mi"][1]) == 2
        assert run(c["si"][0], c["sop"][0]) == 1 and run(c["sop"][0], c["sop"][1], c["si"][0]) == 2, "an interleaved plan and its planar-output sibling"
        assert run(c["pl"][0], c["pl"][1], c["pl"][0]) == 2, "the same converter twice ends the run"
        assert run(*c["pt"]) == 1 and run(*c["en"]) == 1 and run(*c["wpt"]) == 1, "passthrough and the endian plan stay single"
        assert run(c["pl"][0], c["pl"][1], src=[1, None]) == 1 and run(c["pl"][0], c["pl"][1], src=[None, 1]) == 1, "a NULL input neither joins nor starts a run"
        assert run(c["pl"][0], c["pl"][1], frames=[8, 1 << 30]) == 1 and run(c["pl"][0], c["pl"][1], frames=[(1 << 30) - 1, 8]) == 2
        many = [be.new(PLANAR) for _ in range(70)]
        assert run(*many) == 64, "no cap below 64 for any shape: every table holds 64 entries"
        for x in many:
            be.free(x)
        r = be.new(Plan("F32LE", "S16LE", il=1, ol=1, in_rate=48000, out_rate=44100, dither_method="tpdf", noise_shaping="high"))
        assert be.run_length([c["pl"][0], r], [1, 1], [8, 8], [8, 7]) == 1, "a resampler inside is part of what a run shares"
        be.free(r)
    finally:
        for v in c.values():
            for x in v:
                be.free(x)


def check_run_rules(be):
    # a mono planar and a mono interleaved converter of otherwise equal arguments: separate runs
    plans = [MONO_P, MONO_P, MONO_I, MONO_I]
    got, _ = both(be, plans, rounds_of(plans, [(33, 12, 33, 12)] * 2, 3))
    assert [c for _, c, _ in got] == [[2, 4, 0, 4]] * 2
    plans = [MONO_P, MONO_I, MONO_P]
    got, _ = both(be, plans, rounds_of(plans, [(33, 12, 5)] * 2, 4))
    assert [c for _, c, _ in got] == [[0, 0, 3, 0]] * 2
    # an interleaved plan next to its planar-output sibling
    plans = [STEREO_I, STEREO_I, STEREO_OP, STEREO_OP, STEREO_I]
    got, _ = both(be, plans, rounds_of(plans, [(33, 12, 5, 67, 9)] * 2, 5))
    assert [c for _, c, _ in got] == [[2, 4, 1, 4]] * 2
    # the same planar converter twice: c0 c1 share the launches, c0's second buffer follows by itself (round 1 one by one on both sides)
    plans, share = [PLANAR] * 3, [0, 1, 0]
    got, _ = both(be, plans, rounds_of(plans, [(67, 40, 33)] * 2, 9), ("many", "single"), share)
    assert got[0][1] == [1, 2, 1, 3]
    # 70 planar streams: 64 + 6
    plans = [STEREO_OP] * 70
    got, _ = both(be, plans, rounds_of(plans, [(13,) * 70], 21))
    assert got[0][1] == [2, 70, 0, 4]


def test_run_rules_on_host(emu_backend):
    check_run_rules(emu_backend)


@pytest.mark.gpu
def test_run_rules_on_device(gpu_backend):
    check_run_rules(gpu_backend)


# ---- F / G. an empty stream inside a run; the refusals ----------------------------------------------------------------------------------------
EDGE_FRAMES = 33
EDGE_PLANS = {
    "planar": PLANAR,
    "wide": Plan("F32LE", "S16LE", in_ch=12, out_ch=4, il=1, ol=1, wide=True, matrix=matrix(4, 12, 7), dither_method="tpdf", noise_shaping="medium"),
}


def first_call_bytes(be, plan, raw):
    c = be.new(plan)
    try:
        blocks, _ = M.call(be, [plan], [c], [(raw, EDGE_FRAMES, EDGE_FRAMES, 0, 0)], "single")
        return blocks[0]
    finally:
        be.free(c)


def check_untouched(be, plan, convs, raws, outs, skip=()):
    """the outputs still hold the guard pattern, and every converter's next single call gives a first call's bytes: its state did not move"""
    for k, b in enumerate(outs.read()):
        assert k in skip or (b == GUARD).all(), k
    for k, c in enumerate(convs):
        if k not in skip:
            blocks, _ = M.call(be, [plan], [c], [(raws[k], EDGE_FRAMES, EDGE_FRAMES, 0, 0)], "single")
            L.same([blocks[0]], [first_call_bytes(be, plan, raws[k])], ("a first call", k))


def check_edges(be, which):
    plan = EDGE_PLANS[which]
    raws = [L.stream(plan.ifmt, plan.in_ch, EDGE_FRAMES, 40 + k) for k in range(3)]
    size = EDGE_FRAMES * plan.out_ch * BYTES[plan.ofmt]

    def setup():
        convs = [be.new(plan) for _ in range(3)]
        ins, outs = M.Bufs(be, [(r, 0) for r in raws]), M.Bufs(be, [(size, 0)] * 3)
        return convs, ins, outs, [ins.ptr(k) for k in range(3)], [outs.ptr(k) for k in range(3)]

    # an empty stream inside a run: skipped, the two around it share their launches
    convs, ins, outs, srcs, dsts = setup()
    assert be.many(convs, srcs, [EDGE_FRAMES, 0, EDGE_FRAMES], dsts, [EDGE_FRAMES] * 3) == 0
    assert be.debug() == [1, 2, 0, 3]
    blocks = outs.read()
    L.same([blocks[0], blocks[2]], [first_call_bytes(be, plan, raws[0]), first_call_bytes(be, plan, raws[2])], "around the empty stream")
    check_untouched(be, plan, convs, raws, outs, skip=(0, 2))
    for c in convs:
        be.free(c)

    # refusals: GSTAMD_ERR_INVALID before anything is launched
    n3 = [EDGE_FRAMES] * 3
    for what, args in (("a NULL converter", lambda cv, s, d: ([cv[0], None, cv[2]], s, n3, d, n3)),
                       ("a NULL out[i]", lambda cv, s, d: (cv, s, n3, [d[0], d[1], None], n3)),
                       ("a NULL input without a resampler", lambda cv, s, d: (cv, [s[0], s[1], None], n3, d, n3)),
                       ("in_frames != out_frames without a resampler", lambda cv, s, d: (cv, s, n3, d, [EDGE_FRAMES, EDGE_FRAMES, EDGE_FRAMES - 1]))):
        convs, ins, outs, srcs, dsts = setup()
        assert be.many(*args(convs, srcs, dsts)) == ERR_INVALID, what
        assert be.debug() == [0, 0, 0, 0], what
        check_untouched(be, plan, convs, raws, outs)
        for c in convs:
            be.free(c)


@pytest.mark.parametrize("which", sorted(EDGE_PLANS))
def test_empty_stream_and_refusals_on_host(emu_backend, which):
    check_edges(emu_backend, which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(EDGE_PLANS))
def test_empty_stream_and_refusals_on_device(gpu_backend, which):
    check_edges(gpu_backend, which)


# ---- H. emulator and device agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_emulator_and_device_agree(gpu_backend, emu_lib):
    emu = EmuMany(emu_lib)
    for name in sorted(PLANS):
        if name[0] in "ab":
            (_, on_host), (_, on_device) = case_abc(emu, name), case_abc(gpu_backend, name)
            M.check_equal(on_device, on_host, name)
            assert [c for _, c, _ in on_device] == [c for _, c, _ in on_host], name
    for name in sorted(E_PLANS):
        (_, on_host), (_, on_device) = case_e(emu, name), case_e(gpu_backend, name)
        M.check_equal(on_device, on_host, name)
        assert [c for _, c, _ in on_device] == [c for _, c, _ in on_host], name
