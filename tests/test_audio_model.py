"""Every FIR kernel of the resampler (k_fir, k_history, k_fir_lds, k_fir_lds_many, k_fir_interp_lds, k_fir_interp_lds_many) against the float64
model of tests/resample_model.py, which shares no code with the product: not the filter design, not the tap tables, not the phase walk, not the
history bookkeeping.  Nothing here needs the reference tree.

A. the model is the reference's filter: the golden float streams (bytes the reference produced) lie within the bound of the model;
B. one stream at the kernels' edges: formats, modes, the narrowest and the widest windows, output counts around the block size, tiny buffers, the
   drain, channel counts, non-interleaved sides, qualities, methods, and the old two-launch path;
C. 3 and 70 streams through resample_many, every stream against a model instance of its own;
D. the bounds tell a wrong filter from the right one (model only).

The tolerances are resample_model.tolerance: derived from the number formats, not from what the kernels give.  Every check of B and C
runs on the host emulator (-m "not gpu") and on the device (-m gpu) and prints its largest error / tolerance."""
import contextlib

import numpy as np
import pytest

import cases
import resample_model as M
from gstreamer_amd import audio as A
from test_audio_interp import GOLDEN, Emu, be, feed, feed_many, fits_lds  # noqa: F401  (be is a fixture)

FORMATS = ("S16LE", "S32LE", "F32LE", "F64LE")
MODES = ("full", "linear", "cubic")           # a FULL table (blended with cubic weights when it is built), INTERPOLATED linear, INTERPOLATED cubic
# per mode: 160 / 147 phases or the interpolated neighbour; samp_inc 0; the longest windows (samp_inc 12 and 6, 744 and 376 taps)
RATES = {"full": ((48000, 44100), (44100, 48000), (96000, 8000)), "interpolated": ((48000, 44101), (44100, 48001), (48000, 7999))}
COUNTS = (1, 63, 64, 65, 129)                 # output frames of one buffer around the 64 frames of a workgroup


def kind_of(mode):
    return "full" if mode == "full" else "interpolated"


def signal(fmt, ch, n, seed, amp=0.25):
    """amp * U(-1, 1) noise, rounded into the format"""
    x = cases.audio_buffer("F64LE", ch, n, seed) * amp
    if fmt in M.PREC:
        return np.rint(x * 2.0 ** M.PREC[fmt]).astype(cases.AUDIO_DTYPES[fmt])
    return x.astype(cases.AUDIO_DTYPES[fmt])


def model_plan(fmt, mode, rates, method="kaiser", quality=4):
    if method not in ("kaiser", "blackman-nuttall"):
        return M.Plan(fmt, rates[0], rates[1], method, quality)
    return M.Plan(fmt, rates[0], rates[1], method, quality, kind_of(mode), "linear" if mode == "linear" else "cubic")


def product_options(mode, rates, method="kaiser", quality=4):
    if method not in ("kaiser", "blackman-nuttall"):
        return A.options(method, quality, rates[0], rates[1])
    if mode == "full":
        return A.options(method, quality, rates[0], rates[1], filter_mode="full")
    return A.options(method, quality, rates[0], rates[1], filter_mode="interpolated", filter_interpolation=mode)


def compare(plan, got, res, what):
    """got [n][ch] of the format against the model's buffer: the largest error / tolerance (0 for an empty buffer)"""
    assert got.shape == res.y.shape, what
    if plan.nearest:
        assert got.tobytes() == res.y.astype(got.dtype).tobytes(), what
        return 0.0
    err, tol = np.abs(got.astype(np.float64) - res.y), M.tolerance(plan, res)
    ratio = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    assert (err <= tol).all(), (what, "error / tolerance", ratio, "worst error", float(err.max()))
    return ratio


def report(be_name, fmt, mode, path, ratio):
    print("model-ratio %s %s %s %s %.4f" % (be_name, fmt, mode, path, ratio))


# ---- A. the golden float streams ---------------------------------------------------------------------------------------------------------------
FLOAT_CASES = [c for c in cases.AUDIO_CASES if c[1] in ("F32LE", "F64LE")]


@pytest.mark.parametrize("case", FLOAT_CASES, ids=lambda c: c[0])
def test_golden_float_streams_lie_within_the_bound_of_the_model(native_lib, emu_lib, case):
    """the emulator's bytes are the reference's (their sha256 is the golden one) and they lie within the float bound of the model: the model is
    the reference's filter, for every method, for full and interpolated tables"""
    assert len(FLOAT_CASES) == 18
    emu = Emu(emu_lib)
    name, fmt, ch, ir, orr, method, quality, bufs = case
    dt = cases.AUDIO_DTYPES[fmt]
    mode, interp = cases.AUDIO_FILTER.get(name, ("auto", "cubic"))
    plan = M.Plan(fmt, ir, orr, method, quality, mode, interp)
    model = M.Resampler(plan, ch)
    h = emu.new(fmt, ch, ir, orr, method, A.options(method, quality, ir, orr, **cases.audio_filter_kwargs(name)))
    assert emu.filter_mode(h) == A.FILTER_MODE[plan.mode] and emu.latency(h) == plan.latency
    chunks, counts, worst = [], [], 0.0
    for i, n in enumerate(list(bufs) + [None]):
        data = None if n is None else cases.audio_buffer(fmt, ch, n, cases.case_seed(name) + i)
        n_in = plan.latency if n is None else n
        assert emu.out_frames(h, n_in) == model.out_frames(n_in), (name, i)
        got, _ = feed(emu, h, dt, ch, data, n_in)
        worst = max(worst, compare(plan, got, model.resample(data, n_in), (name, i)))
        chunks.append(got.reshape(-1))
        counts.append(got.shape[0])
    emu.free(h)
    assert counts == GOLDEN[name]["out_frames"]
    assert cases.sha(np.concatenate(chunks)) == GOLDEN[name]["sha256"]
    report("emu", fmt, "golden-" + plan.mode, "A", worst)


# ---- B. one stream at the kernels' edges --------------------------------------------------------------------------------------------------------
_edge_models = {}


def edge_model(fmt, mode, rates, ch, method="kaiser", quality=4):
    """the stream of B through the model, once per (format, mode, rates, channels, method, quality): (plan, [(n_in, data or None, Result)]).
    A first buffer of latency + 10 frames; buffers cut to give 1, 63, 64, 65 and 129 output frames; buffers of 1 and of 3 frames (no output where a
    step of the walk is longer than they are; one to four frames otherwise); a buffer of 200; the drain."""
    key = (fmt, mode, rates, ch, method, quality)
    if key in _edge_models:
        return _edge_models[key]
    plan = model_plan(fmt, mode, rates, method, quality)
    r = M.Resampler(plan, ch)
    bufs = []

    def push(n, silent=False):
        data = None if silent else signal(fmt, ch, n, 9000 + len(bufs))
        bufs.append((n, data, r.resample(data, n)))
        assert r.kept > 0                     # (the hand-over of the history always has frames to move in these streams)

    push(plan.latency + 10)
    for want in COUNTS:
        for _ in range(64):
            n = 1
            while r.out_frames(n) < want:
                n += 1
            if r.out_frames(n) == want:
                break
            push(1)                           # an upsampler makes two frames of some input frames: one frame on, and cut again
        push(n)
        assert bufs[-1][2].y.shape[0] == want
    push(1)
    push(3)
    if plan.samp_inc >= 5:
        assert bufs[-1][2].y.shape[0] == 0 and bufs[-2][2].y.shape[0] == 0
    push(200)
    push(plan.latency, silent=True)
    assert bufs[-1][2].y.shape[0] > 0 or plan.latency <= plan.samp_inc + 1      # (nearest, 3 -> 2: one silent frame may fall between two outputs)
    _edge_models[key] = (plan, bufs)
    return _edge_models[key]


def check_edge_stream(be, fmt, mode, rates, ch=2, layout=(False, False), method="kaiser", quality=4, old=False):
    plan, bufs = edge_model(fmt, mode, rates, ch, method, quality)
    dt = cases.AUDIO_DTYPES[fmt]
    opts = product_options(mode, rates, method, quality)
    staged = not old and fits_lds(be, fmt, ch, rates[0], rates[1], method, opts)      # (0 bytes, so not staged: nearest)
    worst = 0.0
    with (be.knob("GSTAMD_NO_FIR_LDS") if old else contextlib.nullcontext()):
        h = be.new(fmt, ch, rates[0], rates[1], method, opts, in_planar=layout[0], out_planar=layout[1])
        assert be.filter_mode(h) == A.FILTER_MODE[plan.mode] and be.latency(h) == plan.latency
        for i, (n, data, res) in enumerate(bufs):
            what = (be.name, fmt, mode, rates, ch, layout, method, quality, old, "buffer", i)
            on = res.y.shape[0]
            assert be.out_frames(h, n) == on, what
            got, rec = feed(be, h, dt, ch, data, n, layout)
            worst = max(worst, compare(plan, got, res, what))
            # one launch serves a buffer whose plan is staged in LDS; k_fir + k_history otherwise; k_history alone for a buffer without output
            assert rec == (([1, int(plan.mode == "interpolated"), 0, 1] if staged else [2, 0, 0, 1]) if on else [1, 0, 0, 1]), (what, rec)
        be.free(h)
    report(be.name, fmt, mode if method == "kaiser" else "method-" + method, "two-launch" if not staged else "one-launch", worst)
    return staged


@pytest.mark.parametrize("pair", (0, 1, 2), ids=("48k_44k1", "samp_inc_0", "longest_window"))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edge_stream_formats_modes_and_rates(be, fmt, mode, pair):
    check_edge_stream(be, fmt, mode, RATES[kind_of(mode)][pair])


@pytest.mark.parametrize("ch", (1, 3, 8))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edge_stream_channel_counts(be, fmt, mode, ch):
    check_edge_stream(be, fmt, mode, RATES[kind_of(mode)][0], ch=ch)


@pytest.mark.parametrize("layout", [(True, False), (False, True), (True, True)], ids=["planar_in", "planar_out", "planar_both"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edge_stream_non_interleaved_sides(be, fmt, mode, layout):
    check_edge_stream(be, fmt, mode, RATES[kind_of(mode)][0], ch=3, layout=layout)


@pytest.mark.parametrize("method,quality", [("kaiser", 0), ("kaiser", 10), ("blackman-nuttall", 4)], ids=["kaiser_q0", "kaiser_q10", "blackman_nuttall"])
@pytest.mark.parametrize("mode", ("full", "cubic"))
@pytest.mark.parametrize("fmt", ("F32LE", "S32LE"))
def test_edge_stream_qualities_and_windows(be, fmt, mode, method, quality):
    check_edge_stream(be, fmt, mode, RATES[kind_of(mode)][0], method=method, quality=quality)


@pytest.mark.parametrize("rates", [(48000, 44100), (48000, 32000)], ids=["48k_44k1", "3_to_2"])
@pytest.mark.parametrize("method", ("cubic", "linear", "nearest"))
@pytest.mark.parametrize("fmt", ("F32LE", "S16LE"))
def test_edge_stream_methods_without_a_sinc(be, fmt, method, rates):
    """taps evaluated directly per phase (4 and 2 of them; 6 and 3 for 3 -> 2, rows padded to a multiple of 4); nearest: equal bytes"""
    check_edge_stream(be, fmt, "full", rates, method=method)


@pytest.mark.parametrize("pair", (0, 1, 2), ids=("48k_44k1", "samp_inc_0", "longest_window"))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", ("F64LE", "S32LE"))
def test_edge_stream_through_k_fir_and_k_history(be, fmt, mode, pair):
    """GSTAMD_NO_FIR_LDS: the two-launch path, elsewhere the yardstick of the staged kernels, judged by the model itself"""
    assert not check_edge_stream(be, fmt, mode, RATES[kind_of(mode)][pair], old=True)


def test_edge_streams_past_the_lds_budget_take_two_launches(be):
    """the plans of the grid above that do not fit 64 KB of LDS (so that k_fir + k_history are also reached without the knob)"""
    assert not check_edge_stream(be, "F64LE", "linear", (48000, 7999))
    assert not check_edge_stream(be, "S32LE", "full", (96000, 8000))
    assert check_edge_stream(be, "S32LE", "cubic", (48000, 7999))


# ---- C. many streams ------------------------------------------------------------------------------------------------------------------------------
_many_models = {}
MANY_FRAMES = 256


def many_model(fmt, mode, n):
    """n streams, each with its own seed, head start (37 * (i % 9) + 5 frames fed singly) and amplitude (0.05 .. 0.25: a neighbour's samples miss the
    bound by orders of magnitude), then two rounds of 256 frames: (plan, per stream [(n_in, data, Result)] * 3)"""
    key = (fmt, mode, n)
    if key not in _many_models:
        rates = RATES[kind_of(mode)][0]
        plan = model_plan(fmt, mode, rates)
        streams = []
        for i in range(n):
            r = M.Resampler(plan, 2)
            start = 37 * (i % 9) + 5
            sig = signal(fmt, 2, start + 2 * MANY_FRAMES, 7000 + i, amp=0.05 + 0.02 * ((7 * i) % 11))
            cuts = [(0, start), (start, start + MANY_FRAMES), (start + MANY_FRAMES, start + 2 * MANY_FRAMES)]
            streams.append([(b - a, sig[a:b], r.resample(sig[a:b], b - a)) for a, b in cuts])
        _many_models[key] = (plan, rates, streams)
    return _many_models[key]


@pytest.mark.parametrize("n", (3, 70))
@pytest.mark.parametrize("fmt,mode", [("F32LE", "full"), ("S16LE", "full"), ("F32LE", "cubic"), ("S32LE", "cubic")])
def test_many_streams_each_against_its_own_model(be, fmt, mode, n):
    """k_fir_lds_many (full tables) and k_fir_interp_lds_many: at most 64 streams share a launch, so 70 take two"""
    plan, rates, streams = many_model(fmt, mode, n)
    dt = cases.AUDIO_DTYPES[fmt]
    opts = product_options(mode, rates)
    hs = [be.new(fmt, 2, rates[0], rates[1], "kaiser", opts) for _ in range(n)]
    worst = 0.0
    for i, h in enumerate(hs):
        n_in, data, res = streams[i][0]
        assert be.out_frames(h, n_in) == res.y.shape[0]
        worst = max(worst, compare(plan, feed(be, h, dt, 2, data, n_in)[0], res, (fmt, mode, "head start", i)))
    launches = (n + 63) // 64
    for rnd in (1, 2):
        for i, h in enumerate(hs):
            assert be.out_frames(h, MANY_FRAMES) == streams[i][rnd][2].y.shape[0] > 0
        got, rec = feed_many(be, hs, dt, 2, [s[rnd][1] for s in streams], [MANY_FRAMES] * n)
        assert rec == [launches, launches if plan.mode == "interpolated" else 0, n, 0], rec
        for i in range(n):
            worst = max(worst, compare(plan, got[i], streams[i][rnd][2], (fmt, mode, "round", rnd, "stream", i)))
    for h in hs:
        be.free(h)
    report(be.name, fmt, mode, "many-%d" % n, worst)


# ---- D. the bounds discriminate -------------------------------------------------------------------------------------------------------------------
def wrong_model_ratio(fmt, mode, rates, wrong):
    """the stream of B through a deliberately wrong model: its largest distance from the true model's output, in tolerances of the true one"""
    plan, bufs = edge_model(fmt, mode, rates, 2)
    r = M.Resampler(plan, 2, wrong=wrong)
    worst = 0.0
    for n, data, res in bufs:
        bad = r.resample(data, n)
        assert bad.y.shape == res.y.shape
        err, tol = np.abs(bad.y - res.y), M.tolerance(plan, res)
        if (tol > 0).any():
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
    return worst


@pytest.mark.parametrize("fmt,mode,rates", [("F64LE", "cubic", (48000, 44101)), ("S32LE", "full", (48000, 44100)), ("F32LE", "full", (48000, 44100))],
                         ids=["F64", "S32", "F32"])
def test_bounds_tell_a_wrong_filter_from_the_right_one(fmt, mode, rates):
    """A phase one step ahead (1 / 44101 or 1 / 147 of a frame) and a window one frame ahead miss the bound by more than 100 times; a dropped end
    tap misses it for F64 and S32.  F32 cannot see that tap: it is about 1e-5 of the filter's gain, which is what 2^-24 times the tolerance's
    factor of 32 times A comes to - so that check is left out for F32."""
    assert wrong_model_ratio(fmt, mode, rates, "phase") > 100
    assert wrong_model_ratio(fmt, mode, rates, "window") > 100
    if fmt != "F32LE":
        assert wrong_model_ratio(fmt, mode, rates, "tap") > 1
