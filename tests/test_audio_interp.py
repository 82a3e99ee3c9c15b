"""INTERPOLATED filter mode through its LDS-staged kernel: k_fir_interp_lds, one launch per call, and k_fir_interp_lds_many behind
gstamd_audio_resampler_resample_many.

Nothing here needs the reference tree.  Expected bytes come from two places only: the reference's hashes in tests/golden/audio_golden.json, and the
same stream through the old path (k_fir + k_history, the one-lane body fir_output) with GSTAMD_NO_FIR_LDS set.  The launch record of every call
(gstamd_audio_resampler_debug_launches: launches, of those interpolated LDS launches, streams batched, streams one by one) is checked with the
bytes, so the old path behind the new name fails too.

A. the golden interpolated streams and update streams;  B. the edges of the block geometry against the old path;  C. a plan past the LDS budget
falls back;  D. many streams;  E. the converter's samples_many;  F. emulator and device agree byte for byte (GPU only).

Every check runs twice: -m "not gpu" on the host emulator (tests/emu/emu_audio_interp.cpp walks the grid block by block and lane by lane),
-m gpu through the C ABI on the device.  Output buffers sit between guard bytes that must survive."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest

import cases
from gstreamer_amd import audio as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "audio_golden.json")))
GUARD, GUARD_BYTES = 0xA5, 64
INTERPOLATED = A.FILTER_MODE["interpolated"]
LDS_BUDGET = 64 * 1024


# ---- backends --------------------------------------------------------------------------------------------------------------------------
class Emu:
    """tests/emu/emu_audio_interp.cpp"""
    name = "emu"

    def __init__(self, emu):
        self.e = emu
        pp, ps = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        emu.emu_interp_new.restype = C.c_void_p
        emu.emu_interp_new.argtypes = [C.c_int] * 6 + [C.POINTER(A.ResamplerOptions), C.POINTER(C.c_int)]
        emu.emu_interp_free.argtypes = [C.c_void_p]
        for f in (emu.emu_interp_get_out_frames, emu.emu_interp_get_max_latency, emu.emu_interp_lds_bytes):
            f.restype = C.c_size_t
        emu.emu_interp_get_out_frames.argtypes = [C.c_void_p, C.c_size_t]
        emu.emu_interp_get_max_latency.argtypes = [C.c_void_p]
        emu.emu_interp_lds_bytes.argtypes = [C.c_void_p]
        emu.emu_interp_filter_mode.argtypes = [C.c_void_p]
        emu.emu_interp_update.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(A.ResamplerOptions)]
        emu.emu_interp_resample.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        emu.emu_interp_resample_many.argtypes = [C.c_int, pp, pp, ps, pp, ps]
        emu.emu_interp_launches.argtypes = [C.POINTER(C.c_int32), C.c_int]

    def new(self, fmt, ch, ir, orr, method="kaiser", opts=None, in_planar=False, out_planar=False):
        st = C.c_int(0)
        h = self.e.emu_interp_new(A.METHODS[method], (1 if in_planar else 0) | (2 if out_planar else 0), A.FORMATS[fmt], ch, ir, orr,
                                  C.byref(opts) if opts is not None else None, C.byref(st))
        assert h, st.value
        return h

    def free(self, h):
        self.e.emu_interp_free(h)

    def out_frames(self, h, n):
        return self.e.emu_interp_get_out_frames(h, n)

    def latency(self, h):
        return self.e.emu_interp_get_max_latency(h)

    def filter_mode(self, h):
        return self.e.emu_interp_filter_mode(h)

    def update(self, h, ir, orr, opts):
        assert self.e.emu_interp_update(h, ir, orr, C.byref(opts) if opts is not None else None) == 0

    def upload(self, host):
        a = host.copy()
        return a, a.ctypes.data

    def download(self, keep):
        return keep.copy()

    def resample(self, h, src, n, dst, on):
        self.e.emu_interp_resample(h, src, n, dst, on)

    def many(self, hs, srcs, nin, dsts, nout):
        n = len(hs)
        assert self.e.emu_interp_resample_many(n, (C.c_void_p * n)(*hs), (C.c_void_p * n)(*srcs), (C.c_size_t * n)(*nin), (C.c_void_p * n)(*dsts),
                                               (C.c_size_t * n)(*nout)) == 0

    def record(self):
        buf = (C.c_int32 * 4)()
        assert self.e.emu_interp_launches(buf, 4) == 4
        return list(buf)

    @contextlib.contextmanager
    def knob(self, name):
        assert name not in os.environ
        os.environ[name] = "1"
        try:
            yield
        finally:
            del os.environ[name]


class Dev:
    """the HIP kernels through the C ABI"""
    name = "gpu"

    def __init__(self, dev):
        self.dev = dev

    def new(self, fmt, ch, ir, orr, method="kaiser", opts=None, in_planar=False, out_planar=False):
        return A.AudioResampler(fmt, ch, ir, orr, method, opts, in_planar=in_planar, out_planar=out_planar)

    def free(self, r):
        r.free()

    def out_frames(self, r, n):
        return r.get_out_frames(n)

    def latency(self, r):
        return r.get_max_latency()

    def filter_mode(self, r):
        return r.debug()["filter_mode"]

    def update(self, r, ir, orr, opts):
        r.update(ir, orr, opts)

    def upload(self, host):
        import torch
        t = torch.from_numpy(host).to(self.dev)
        return t, t.data_ptr()

    def download(self, keep):
        import torch
        torch.cuda.synchronize()
        return keep.cpu().numpy()

    def resample(self, r, src, n, dst, on):
        r.resample(src, n, dst, on)

    def many(self, rs, srcs, nin, dsts, nout):
        A.resample_many(rs, srcs, nin, dsts, nout)

    def record(self):
        d = A.resample_debug()
        return [d["launches"], d["interp_lds_launches"], d["batched"], d["single"]]

    @contextlib.contextmanager
    def knob(self, name):
        from gstreamer_amd import video as V
        with V.tuning(**{name: 1}):
            yield


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request, native_lib, emu_lib):
    b = Emu(emu_lib) if request.param == "emu" else Dev(request.getfixturevalue("gpu"))
    b.host = Emu(emu_lib)                        # the plan on the host, for the fit rule
    return b


def fits_lds(be, *args, **kw):
    """the fit rule, asked of the host's plan: the plan's staged kernel works in at most 64 KB of LDS"""
    h = be.host.new(*args, **kw)
    n = be.host.e.emu_interp_lds_bytes(h)
    be.host.free(h)
    return 0 < n <= LDS_BUDGET


# ---- one call: the input uploaded, the output between guard bytes ---------------------------------------------------------------------------
def guarded(be, sizes):
    """one allocation with a block of sizes[k] bytes for every stream, GUARD_BYTES of guard pattern around each (blocks start 64-byte aligned)"""
    offs, pos = [], 0
    for s in sizes:
        offs.append(pos + GUARD_BYTES)
        pos += (GUARD_BYTES + s + GUARD_BYTES + 63) // 64 * 64
    keep, base = be.upload(np.full(pos, GUARD, np.uint8))
    return keep, [base + o for o in offs], offs


def read_guarded(be, keep, offs, sizes):
    got = be.download(keep)
    mask = np.ones(got.size, bool)
    for o, s in zip(offs, sizes):
        mask[o: o + s] = False
    assert (got[mask] == GUARD).all(), "guard bytes overwritten"
    return [got[o: o + s].copy() for o, s in zip(offs, sizes)]


def feed(be, h, dt, ch, data, n_in, layout=(False, False)):
    """one _resample call: data [n_in][ch] (None: silence) -> [n_out][ch], the launch record"""
    in_planar, out_planar = layout
    on = be.out_frames(h, n_in)
    src_keep, src = None, None
    if data is not None:
        src_keep, src = be.upload(np.ascontiguousarray(data.T if in_planar else data).view(np.uint8).reshape(-1))
    size = on * ch * np.dtype(dt).itemsize
    keep, ptrs, offs = guarded(be, [size])
    be.resample(h, src, n_in, ptrs[0], on)
    rec = be.record()
    raw = read_guarded(be, keep, offs, [size])[0].view(dt)
    del src_keep
    return (raw.reshape(ch, on).T if out_planar else raw.reshape(on, ch)).copy(), rec


def feed_many(be, hs, dt, ch, datas, n_ins):
    """one _resample_many call over interleaved streams: the outputs and the launch record"""
    ons = [be.out_frames(h, n) for h, n in zip(hs, n_ins)]
    ups = [None if d is None else be.upload(np.ascontiguousarray(d).view(np.uint8).reshape(-1)) for d in datas]
    sizes = [on * ch * np.dtype(dt).itemsize for on in ons]
    keep, ptrs, offs = guarded(be, sizes)
    be.many(hs, [None if u is None else u[1] for u in ups], n_ins, ptrs, ons)
    rec = be.record()
    return [b.view(dt).reshape(on, ch).copy() for b, on in zip(read_guarded(be, keep, offs, sizes), ons)], rec


def interp_options(kind, quality, ir, orr, method="kaiser"):
    return A.options(method, quality, ir, orr, filter_mode="interpolated", filter_interpolation=kind)


# ---- A. goldens ------------------------------------------------------------------------------------------------------------------------------
INTERP_CASES = [c for c in cases.AUDIO_CASES if "_interp_" in c[0]]
INTERP_UPDATE_CASES = [c for c in cases.AUDIO_UPDATE_CASES if c[0] in ("upd_f32_interp_null_options", "upd_f32_full_to_interpolated")]


@pytest.mark.parametrize("case", INTERP_CASES, ids=lambda c: c[0])
def test_golden_interpolated_streams_take_one_interp_lds_launch(be, case):
    """This is the test that fails without the feature: the record entry does not exist there and two launches are issued."""
    assert len(INTERP_CASES) == 9
    name, fmt, ch, ir, orr, method, quality, bufs = case
    dt = cases.AUDIO_DTYPES[fmt]
    h = be.new(fmt, ch, ir, orr, method, A.options(method, quality, ir, orr, **cases.audio_filter_kwargs(name)))
    assert be.filter_mode(h) == INTERPOLATED
    chunks, counts = [], []
    for i, n in enumerate(list(bufs) + [None]):
        data = None if n is None else cases.audio_buffer(fmt, ch, n, cases.case_seed(name) + i)
        got, rec = feed(be, h, dt, ch, data, be.latency(h) if n is None else n)
        assert rec == [1, 1, 0, 1], (name, i, rec)
        chunks.append(got.reshape(-1))
        counts.append(got.shape[0])
    be.free(h)
    assert counts == GOLDEN[name]["out_frames"]
    assert cases.sha(np.concatenate(chunks)) == GOLDEN[name]["sha256"]


@pytest.mark.parametrize("case", INTERP_UPDATE_CASES, ids=lambda c: c[0])
def test_golden_update_streams_through_the_interpolated_kernel(be, case):
    """gst_audio_resampler_update in mid-stream; upd_f32_full_to_interpolated moves a stream from a FULL table to an interpolated one and back:
    one launch per call throughout, an interpolated LDS launch exactly while the plan is interpolated."""
    name, fmt, ch, ir, orr, method, quality, script = case
    dt = cases.AUDIO_DTYPES[fmt]
    h = be.new(fmt, ch, ir, orr, method, A.options(method, quality, ir, orr, **cases.audio_filter_kwargs(name)))
    counts, seen = [], set()

    def do_update(item):
        raw = item.get("raw", (item["in_rate"], item["out_rate"]))
        uo = None
        if cases.audio_update_has_options(item):
            kw = {k: item[k] for k in ("filter_mode", "filter_interpolation") if k in item}
            uo = A.options(method, item.get("quality"), item["in_rate"], item["out_rate"], **kw)
        be.update(h, raw[0], raw[1], uo)

    def do_resample(data, n_in):
        interp = be.filter_mode(h) == INTERPOLATED
        got, rec = feed(be, h, dt, ch, data, n_in)
        assert rec == [1, 1 if interp else 0, 0, 1], (name, len(counts), rec)
        seen.add(interp)
        counts.append(got.shape[0])
        return got

    out = cases.audio_update_stream(case, do_update, do_resample, lambda: be.latency(h))
    be.free(h)
    assert True in seen and (name != "upd_f32_full_to_interpolated" or seen == {True, False})
    assert counts == GOLDEN[name]["out_frames"]
    assert cases.sha(out) == GOLDEN[name]["sha256"]


# ---- B. edges of the block geometry, against the old path -----------------------------------------------------------------------------------
def in_frames_for(be, h, want):
    """the smallest input buffer that yields `want` output frames from h's present state"""
    n = 0
    while be.out_frames(h, n) < want:
        n += 1
    assert be.out_frames(h, n) == want
    return n


def edge_stream(be, fmt, kind, ch=2, rates=(48000, 44101), layout=(False, False), plan="counts", old=False, seed=0):
    """three or more consecutive buffers of one stream; plan: "counts" - output counts 1, 63, 64, 65, 129; "history" - buffers of 1 and 3 frames that
    yield no output, then a drain with in == NULL; "three" - three buffers of 300 frames.  old: through k_fir + k_history (GSTAMD_NO_FIR_LDS)."""
    dt = cases.AUDIO_DTYPES[fmt]
    ir, orr = rates
    with (be.knob("GSTAMD_NO_FIR_LDS") if old else contextlib.nullcontext()):
        h = be.new(fmt, ch, ir, orr, "kaiser", interp_options(kind, 4, ir, orr), in_planar=layout[0], out_planar=layout[1])
        assert be.filter_mode(h) == INTERPOLATED
        outs, recs, k = [], [], 0

        def push(n, silent=False):
            nonlocal k
            data = None if silent else cases.audio_buffer(fmt, ch, n, 4000 + seed + k)
            k += 1
            got, rec = feed(be, h, dt, ch, data, n, layout)
            outs.append(got)
            recs.append((got.shape[0], rec))

        if plan == "counts":
            push(be.latency(h) + 10)                      # past the start-up, so that every later buffer's count is its own
            for want in (1, 63, 64, 65, 129):
                push(in_frames_for(be, h, want))
                assert outs[-1].shape[0] == want
        elif plan == "history":
            push(1)
            push(3)
            assert outs[0].shape[0] == 0 and outs[1].shape[0] == 0
            push(200)
            push(be.latency(h), silent=True)
            assert outs[-1].shape[0] > 0
        else:
            for _ in range(3):
                push(300)
        be.free(h)
    return outs, recs


def check_edges(be, fmt, kind, **kw):
    ir, orr = kw.get("rates", (48000, 44101))
    # (linear tables are oversampled 11 times as much as cubic ones: of these streams the F64 linear ones with 8 channels and with the six times longer
    # filter of 48000 -> 7999 are past the budget and take the old path; every other one must be served by the new kernel)
    fits = fits_lds(be, fmt, kw.get("ch", 2), ir, orr, "kaiser", interp_options(kind, 4, ir, orr))
    assert fits or ((fmt, kind) == ("F64LE", "linear") and (kw.get("ch") == 8 or orr == 7999))
    new, new_recs = edge_stream(be, fmt, kind, **kw)
    old, old_recs = edge_stream(be, fmt, kind, old=True, **kw)
    assert len(new) == len(old)
    for i, (a, b) in enumerate(zip(new, old)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (fmt, kind, kw, "buffer", i)
    assert sum(a.size for a in new) > 0
    for (on, rec), (_, orec) in zip(new_recs, old_recs):
        # a buffer without output launches the history hand-over alone (k_history; s.run_fir does not hold)
        assert rec == (([1, 1, 0, 1] if fits else [2, 0, 0, 1]) if on else [1, 0, 0, 1]), (fmt, kind, kw, rec)
        assert orec == ([2, 0, 0, 1] if on else [1, 0, 0, 1]), (fmt, kind, kw, orec)
    return new


FORMATS = ("S16LE", "S32LE", "F32LE", "F64LE")
KINDS = ("linear", "cubic")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edges_output_counts_around_the_block_size(be, fmt, kind):
    check_edges(be, fmt, kind, plan="counts")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edges_history_only_buffers_and_drain(be, fmt, kind):
    check_edges(be, fmt, kind, plan="history")


@pytest.mark.parametrize("ch", (1, 3, 8))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edges_channel_counts(be, fmt, kind, ch):
    check_edges(be, fmt, kind, plan="three", ch=ch)          # (2 channels: every other edge test)


@pytest.mark.parametrize("layout", [(True, False), (False, True), (True, True)], ids=["planar_in", "planar_out", "planar_both"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edges_non_interleaved_sides(be, fmt, kind, layout):
    check_edges(be, fmt, kind, plan="three", ch=3, layout=layout)


@pytest.mark.parametrize("rates", [(44100, 48001), (48000, 7999)], ids=["samp_inc_0", "samp_inc_6"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edges_smallest_and_widest_window(be, fmt, kind, rates):
    """44100 -> 48001: samp_inc 0, neighbouring frames share their window; 48000 -> 7999: samp_inc 6, the window of a block spans the most"""
    check_edges(be, fmt, kind, plan="three", rates=rates)


# ---- C. fallback ---------------------------------------------------------------------------------------------------------------------------------
# F64, 8 channels, Kaiser quality 10, 48000 -> 44101: its oversampled table alone is past the budget (checked on the host below)
def test_plan_past_the_lds_budget_falls_back_to_two_launches(be):
    opts = interp_options("cubic", 10, 48000, 44101)
    assert not fits_lds(be, "F64LE", 8, 48000, 44101, "kaiser", opts)

    def run(old):
        with (be.knob("GSTAMD_NO_FIR_LDS") if old else contextlib.nullcontext()):
            h = be.new("F64LE", 8, 48000, 44101, "kaiser", opts)
            res = [feed(be, h, np.float64, 8, cases.audio_buffer("F64LE", 8, n, 700 + i), n) for i, n in enumerate((700, 300, 65))]
            be.free(h)
        return res

    new, old = run(False), run(True)
    assert sum(a.shape[0] for a, _ in new) > 0
    for (a, rec), (b, orec) in zip(new, old):
        assert a.tobytes() == b.tobytes()
        assert rec == [2, 0, 0, 1] and orec == [2, 0, 0, 1]


# ---- D. many streams ---------------------------------------------------------------------------------------------------------------------------
MANY_RATES = (48000, 44101)


def many_streams(be, n, fmt="F32LE", kind="cubic", ch=2, frames=256):
    """n streams with a head start of their own each, then two rounds of resample_many; expected: fresh resamplers driven singly"""
    dt = cases.AUDIO_DTYPES[fmt]
    ir, orr = MANY_RATES
    opts = interp_options(kind, 4, ir, orr)
    sigs = [cases.audio_buffer(fmt, ch, 1000, 5000 + i) for i in range(n)]

    def make():
        hs = [be.new(fmt, ch, ir, orr, "kaiser", opts) for _ in range(n)]
        pos = []
        for i, h in enumerate(hs):
            start = 37 * (i % 9) + 5
            feed(be, h, dt, ch, sigs[i][:start], start)
            pos.append(start)
        return hs, pos

    hs, pos = make()
    got, recs = [], []
    for rnd in range(2):
        o, rec = feed_many(be, hs, dt, ch, [sigs[i][pos[i] + rnd * frames: pos[i] + (rnd + 1) * frames] for i in range(n)], [frames] * n)
        got.append(o)
        recs.append(rec)
    for h in hs:
        be.free(h)
    hs, pos = make()
    exp = [[feed(be, h, dt, ch, sigs[i][pos[i] + rnd * frames: pos[i] + (rnd + 1) * frames], frames)[0] for i, h in enumerate(hs)] for rnd in range(2)]
    for h in hs:
        be.free(h)
    return got, exp, recs


@pytest.mark.parametrize("n,record", [(3, [1, 1, 3, 0]), (70, [2, 2, 70, 0])], ids=["3", "70"])
def test_many_interpolated_streams_share_launches(be, n, record):
    got, exp, recs = many_streams(be, n)
    assert recs == [record, record]
    for rnd in range(2):
        assert sum(a.size for a in exp[rnd]) > 0
        for i in range(n):
            assert got[rnd][i].tobytes() == exp[rnd][i].tobytes(), (rnd, i)


def test_many_with_the_knob_goes_one_by_one(be):
    got, exp, _ = many_streams(be, 5, fmt="S16LE", kind="linear")
    with be.knob("GSTAMD_NO_FIR_MANY"):
        slow, _, recs = many_streams(be, 5, fmt="S16LE", kind="linear")
    assert recs == [[5, 5, 0, 5]] * 2
    for rnd in range(2):
        for i in range(5):
            assert got[rnd][i].tobytes() == exp[rnd][i].tobytes() == slow[rnd][i].tobytes()


def mixed_call(be, specs, srcs_of=None):
    """one resample_many over resamplers made from specs = [(kind or "full", in_rate, out_rate)], F32 stereo, 300 frames each; expected bytes: fresh
    resamplers, one _resample each in array order.  Returns got, exp, record."""
    dt, ch, n = np.float32, 2, 300

    def make():
        hs = [be.new("F32LE", ch, ir, orr, "kaiser", A.options("kaiser", 4, ir, orr) if kind == "full" else interp_options(kind, 4, ir, orr))
              for kind, ir, orr in specs]
        for h in hs:                                 # a buffer first: no stream stands at its start
            feed(be, h, dt, ch, cases.audio_buffer("F32LE", ch, 100, 31), 100)
        return hs

    datas = [cases.audio_buffer("F32LE", ch, n, 6000 + k) for k in range(len(specs))]
    if srcs_of:
        datas = srcs_of(datas)
    hs = make()
    got, rec = feed_many(be, hs, dt, ch, datas, [n] * len(hs))
    for h in hs:
        be.free(h)
    hs = make()
    exp = [feed(be, h, dt, ch, d, n)[0] for h, d in zip(hs, datas)]
    for h in hs:
        be.free(h)
    assert sum(e.size for e in exp) > 0
    return got, exp, rec


def test_many_linear_and_cubic_do_not_share_a_run(be):
    got, exp, rec = mixed_call(be, [("cubic", 48000, 44101), ("linear", 48000, 44101), ("cubic", 48000, 44101), ("cubic", 48000, 44101)])
    assert rec == [3, 3, 2, 2]                       # cubic alone, linear alone, a run of two
    for a, b in zip(got, exp):
        assert a.tobytes() == b.tobytes()


def test_many_null_input_inside_a_run_goes_one_by_one(be):
    got, exp, rec = mixed_call(be, [("cubic", 48000, 44101)] * 3, srcs_of=lambda d: [d[0], None, d[2]])
    assert rec == [3, 3, 0, 3]                       # (a run with a NULL input is not batched: the rule as it stands for FULL tables)
    for a, b in zip(got, exp):
        assert a.tobytes() == b.tobytes()


def test_many_full_run_then_interpolated_run(be):
    got, exp, rec = mixed_call(be, [("full", 48000, 44100)] * 2 + [("cubic", 48000, 44101)] * 3)
    assert rec == [2, 1, 5, 0]
    for a, b in zip(got, exp):
        assert a.tobytes() == b.tobytes()


def test_many_same_resampler_twice(be):
    """the second buffer of a resampler depends on its first: the run ends before the repeat.  Streams 0, 1, 0, 1 -> runs (0, 1) and (0, 1)."""
    dt, ch, ir, orr = np.float32, 2, 48000, 44101
    opts = interp_options("cubic", 4, ir, orr)
    datas = [cases.audio_buffer("F32LE", ch, 441, 6100 + k) for k in range(4)]
    hs = [be.new("F32LE", ch, ir, orr, "kaiser", opts) for _ in range(2)]
    exp = [feed(be, hs[k % 2], dt, ch, datas[k], 441)[0] for k in range(4)]
    for h in hs:
        be.free(h)
    hs = [be.new("F32LE", ch, ir, orr, "kaiser", opts) for _ in range(2)]
    ons = [e.shape[0] for e in exp]
    ups = [be.upload(d.view(np.uint8).reshape(-1)) for d in datas]
    sizes = [on * ch * 4 for on in ons]
    keep, ptrs, offs = guarded(be, sizes)
    be.many([hs[0], hs[1], hs[0], hs[1]], [u[1] for u in ups], [441] * 4, ptrs, ons)
    rec = be.record()
    got = read_guarded(be, keep, offs, sizes)
    for h in hs:
        be.free(h)
    assert rec == [2, 2, 4, 0]
    assert sum(sizes) > 0
    for a, b in zip(got, exp):
        assert a.tobytes() == b.tobytes()


# ---- E. the converter ---------------------------------------------------------------------------------------------------------------------------
def converter_backend(be, request):
    import test_audio_convert_many as M
    return M, (M.EmuMany(request.getfixturevalue("emu_lib")) if be.name == "emu" else M.GpuMany(be.dev))


def test_converter_samples_many_batches_its_interpolated_resamplers(be, request):
    """four converters F32 -> S16, 48000 -> 44101 (filter mode auto picks the interpolated table), TPDF dither: samples_many gives the bytes of four
    single _samples calls, and its one resample_many is one batched interpolated launch.  On the host the emulated converter keeps its own emulated
    resampler, so the record is taken from the resampling step of the same four streams through this file's emulator."""
    M, cb = converter_backend(be, request)
    plans = [M.Plan("F32LE", "S16LE", in_rate=48000, out_rate=44101, dither_method="tpdf")] * 4
    rounds = M.make_rounds(plans, (1024, 1000, 300, 1024), 2, 77)
    got = M.drive(cb, plans, rounds, ("many",) * 2)
    if be.name == "gpu":
        assert be.record() == [1, 1, 4, 0]
    exp = M.drive(cb, plans, rounds, ("single",) * 2)
    M.check_equal(got, exp, "converter")
    assert sum(b.size for b in exp[0][0]) > 0
    for _, counters, _ in got:
        assert counters[:3] == [1, 4, 0]
    if be.name == "emu":
        hs = [be.new("F32LE", 2, 48000, 44101, "kaiser", None) for _ in range(4)]
        assert be.filter_mode(hs[0]) == INTERPOLATED
        frames = (1024, 1000, 300, 1024)
        _, rec = feed_many(be, hs, np.float32, 2, [cases.audio_buffer("F32LE", 2, n, 80 + k) for k, n in enumerate(frames)], list(frames))
        for h in hs:
            be.free(h)
        assert rec == [1, 1, 4, 0]


# ---- F. agreement ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ("F32LE", "S32LE"))
def test_emulator_and_device_agree(native_lib, emu_lib, gpu, fmt):
    """B's cubic streams: what the lane-by-lane walk on the host gives is what the device gives, byte for byte"""
    host, dev = Emu(emu_lib), Dev(gpu)
    for kw in (dict(plan="counts"), dict(plan="history"), dict(plan="three", ch=3, layout=(True, True)), dict(plan="three", rates=(48000, 7999)),
               dict(plan="three", rates=(44100, 48001))):
        a, _ = edge_stream(host, fmt, "cubic", **kw)
        b, _ = edge_stream(dev, fmt, "cubic", **kw)
        assert len(a) == len(b) and sum(x.size for x in a) > 0
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (fmt, kw)
