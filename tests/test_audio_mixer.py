"""audiomixer: many streams summed into one buffer by one launch - gstamd_audio_mixer_mix / k_audio_mix.

Nothing here needs the reference tree.  The expected bytes of every case come from `model` below: a numpy restatement, written from DESIGN
3.9.1 alone, of gst_audio_mixer_aggregate_one_buffer and the C backups of audiomixer_orc_add_* / _add_volume_* - one pass over the output per
input, in array order, int64 for the widened integer arithmetic, element-wise float32 / float64 operations with ORC's denormal flush done with
bit masks.  It imports nothing from gstreamer_amd/csrc and does not call the emulator.  Outputs are compared as bytes, with no tolerance.  The
record of every call (launches, inputs mixed, inputs skipped) is checked with the bytes.

1. piece and workgroup edges;  2. alignment of the output and of every input;  3. windows;  4. the order is observable;  5. volumes and the two
clamps;  6. floats;  7. input counts past one launch;  8. refusals;  9. emulator and device agree (GPU only);  10. behind the batched converter
on one stream.

The cases are grouped into four tests (each names format, channels and frame count in its assertion).  Every one runs twice: -m "not gpu" on the host emulator (tests/emu/emu_audio_mix.cpp walks the grid lane by lane with the library's launch
plan), -m gpu through the C ABI on the device.  The output and every input sit inside one allocation between guard bytes; the output is
pre-filled with the guard pattern, and after the call every byte outside it must be what it was."""
import ctypes as C
import sys
import zlib

import numpy as np
import pytest

from gstreamer_amd import audio as A
import test_audio_convert_many as M

GUARD, GUARD_BYTES = 0xA5, 64
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2        # include/gstamd_video.h; checked against the binding in the GPU tests
DT = {"S16LE": np.int16, "S32LE": np.int32, "F32LE": np.float32, "F64LE": np.float64}
FORMATS = list(DT)
DBL_MIN = sys.float_info.min


# ---- the model: DESIGN 3.9.1 ---------------------------------------------------------------------------------------------------------------
def fl(x):
    """ORC's denormal flush: a value whose exponent field is zero keeps only its sign bit"""
    if x.dtype == np.float32:
        b = x.view(np.uint32)
        return np.where((b & np.uint32(0x7f800000)) == 0, b & np.uint32(0xff800000), b).view(np.float32)
    b = x.view(np.uint64)
    return np.where((b & np.uint64(0x7ff0000000000000)) == 0, b & np.uint64(0xfff0000000000000), b).view(np.float64)


def skipped(i):
    return bool(i["mute"]) or i["vol"] < DBL_MIN or i["frames"] == 0 or i["data"] is None


def add_one(fmt, d, s, vol):
    """one input onto the running sum, the table of DESIGN 3.9.1"""
    if fmt in ("S16LE", "S32LE"):
        bits, shift = (16, 11) if fmt == "S16LE" else (32, 27)
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        t = s.astype(np.int64)
        if vol != 1.0:
            v = int(vol * float(1 << shift))            # truncation
            t = np.clip((t * v) >> shift, lo, hi)       # arithmetic shift, saturating narrow
        return np.clip(d.astype(np.int64) + t, lo, hi).astype(d.dtype)
    dt = d.dtype.type
    with np.errstate(all="ignore"):
        t = fl(s)
        if vol != 1.0:
            v = fl(np.array([vol]).astype(dt))[0]       # (float) volume for F32, volume itself for F64
            t = fl(t * v)
        return fl(fl(d) + fl(t))


def model(fmt, ch, out_frames, ins):
    d = np.zeros(out_frames * ch, DT[fmt])
    for i in ins:
        if skipped(i):
            continue
        lo, n = i["off"] * ch, i["frames"] * ch
        d[lo: lo + n] = add_one(fmt, d[lo: lo + n], i["data"][:n], i["vol"])
    return d


# ---- backends ---------------------------------------------------------------------------------------------------------------------------------
class Emu:
    """tests/emu/emu_audio_mix.cpp"""
    name = "emu"

    def __init__(self, emu):
        self.e = emu
        emu.emu_audio_mixer_mix.argtypes = [C.c_int, C.c_int, C.POINTER(A.MixerInput), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        emu.emu_audio_mixer_debug_launches.argtypes = [C.POINTER(C.c_int32), C.c_int]

    def upload(self, host):
        a = np.zeros(host.size + 64, np.uint8)
        o = (-a.ctypes.data) % 64
        a[o: o + host.size] = host
        return (a, o, host.size), a.ctypes.data + o

    def download(self, keep):
        a, o, n = keep
        return a[o: o + n].copy()

    def mix_raw(self, fmt, ch, arr, n, out, out_frames, stream=None):
        return self.e.emu_audio_mixer_mix(fmt, ch, arr, n, out, out_frames, None)

    def mix(self, fmt, ch, inputs, out, out_frames, stream=None):
        return self.mix_raw(A.AFMT[fmt], ch, A.mixer_inputs(inputs), len(inputs), out, out_frames)

    def record(self):
        buf = (C.c_int32 * 4)()
        assert self.e.emu_audio_mixer_debug_launches(buf, 4) == 4 and buf[3] == 0
        return list(buf)[:3]


class Dev:
    """k_audio_mix through the C ABI and its Python mirror"""
    name = "gpu"

    def __init__(self, dev):
        from gstreamer_amd import video as V
        assert (V.OK, V.ERR_INVALID, V.ERR_UNSUPPORTED) == (OK, ERR_INVALID, ERR_UNSUPPORTED)
        self.dev = dev

    def upload(self, host):
        import torch
        t = torch.zeros(host.size + 64, dtype=torch.uint8, device=self.dev)
        o = (-t.data_ptr()) % 64
        t[o: o + host.size] = torch.from_numpy(host).to(self.dev)
        return (t, o, host.size), t.data_ptr() + o

    def download(self, keep):
        import torch
        t, o, n = keep
        torch.cuda.synchronize()
        return t.cpu().numpy()[o: o + n].copy()

    def mix_raw(self, fmt, ch, arr, n, out, out_frames, stream=None):
        return A._mix_lib().gstamd_audio_mixer_mix(fmt, ch, arr, n, out, out_frames, stream)

    def mix(self, fmt, ch, inputs, out, out_frames, stream=None):
        from gstreamer_amd import video as V
        try:
            A.mixer_mix(fmt, ch, inputs, out, out_frames, stream)
        except V.GstAmdError as e:
            assert str(e)
            return e.code
        return OK

    def record(self):
        d = A.mixer_debug()
        return [d["launches"], d["mixed"], d["skipped"]]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request, native_lib, emu_lib):
    return Emu(emu_lib) if request.param == "emu" else Dev(request.getfixturevalue("gpu"))


# ---- one call: the output and every input inside one allocation, between guard bytes ----------------------------------------------------------
def inp(data, off, frames=None, vol=1.0, mute=False, mis=0, ch=1):
    """one input: data a flat sample array (None: a NULL pointer), landing at output frame off; mis: samples its pointer sits past a 16-byte boundary"""
    return {"data": data, "off": off, "frames": (0 if data is None else data.size // ch) if frames is None else frames, "vol": vol, "mute": mute, "mis": mis}


class Scene:
    """block 0 is the output (out_mis samples past a 16-byte boundary, pre-filled with the guard pattern), block 1 + k input k's samples; every block
    has GUARD_BYTES or more of guard pattern on both sides"""

    def __init__(self, be, fmt, ch, out_frames, ins, out_mis=0):
        self.be, self.fmt, self.ch, self.out_frames, self.ins = be, fmt, ch, out_frames, ins
        bps = np.dtype(DT[fmt]).itemsize
        self.out_size = out_frames * ch * bps
        blocks = [(None, self.out_size, out_mis * bps)] + [(i["data"], 0 if i["data"] is None else i["data"].size * bps, i["mis"] * bps) for i in ins]
        self.offs, pos = [], 0
        for _, size, mis in blocks:
            pos = (pos + GUARD_BYTES + 63) // 64 * 64 + mis
            self.offs.append(pos)
            pos += size
        self.image = np.full(pos + GUARD_BYTES, GUARD, np.uint8)
        for (data, size, _), o in zip(blocks, self.offs):
            if data is not None:
                self.image[o: o + size] = np.ascontiguousarray(data).view(np.uint8)
        self.keep, self.base = be.upload(self.image)
        assert self.base % 64 == 0
        self.out = self.base + self.offs[0]
        self.inputs = [A.MixerInput(None if i["data"] is None else self.base + o, i["off"], i["frames"], i["vol"], int(i["mute"]), 0)
                       for i, o in zip(ins, self.offs[1:])]

    def read(self):
        """the output's bytes, after checking that nothing else changed: the guards, and the inputs"""
        got = self.be.download(self.keep)
        o, n = self.offs[0], self.out_size
        assert (got[:o] == self.image[:o]).all() and (got[o + n:] == self.image[o + n:]).all(), "bytes outside the output changed"
        return got[o: o + n]

    def run(self, stream=None):
        assert self.be.mix(self.fmt, self.ch, self.inputs, self.out, self.out_frames, stream) == OK
        return self.read()


def check(be, fmt, ch, out_frames, ins, out_mis=0, launches=1):
    """run one scene; bytes against the model, the record against the inputs"""
    got = Scene(be, fmt, ch, out_frames, ins, out_mis).run()
    exp = model(fmt, ch, out_frames, ins)
    assert got.tobytes() == exp.tobytes(), (be.name, fmt, ch, out_frames, int(np.argmax(got != exp.view(np.uint8))))
    n_skip = sum(skipped(i) for i in ins)
    assert be.record() == [launches, len(ins) - n_skip, n_skip]
    return exp


def signal(rng, fmt, n, loud=True):
    """integers over the full range (sums of two clamp often), floats around +-1"""
    if fmt in ("S16LE", "S32LE"):
        info = np.iinfo(DT[fmt])
        a = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True)
        return (a if loud else a // 8).astype(DT[fmt])
    return rng.standard_normal(n).astype(DT[fmt])


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- 1. piece and workgroup edges ---------------------------------------------------------------------------------------------------------------
def piece_and_workgroup_edges(be, fmt, ch):
    """three inputs over the whole buffer; frame counts around a piece, a workgroup and two; 3 channels never line a frame up with a piece"""
    rng = rng_for("edges", fmt, ch)
    for out_frames in (1, 3, 255, 256, 257, 1023, 1025):
        ins = [inp(signal(rng, fmt, out_frames * ch), 0, vol=v, ch=ch) for v in (1.0, 0.5, 1.0)]
        check(be, fmt, ch, out_frames, ins)


# ---- 2. alignment ---------------------------------------------------------------------------------------------------------------------------------
def alignment(be, fmt, ch):
    """the output one sample past a 16-byte boundary, input pointers 0 .. 3 samples past one, odd and even out_offsets: every relative alignment
    of an input to the output's pieces, in workgroups whose pieces are all whole (four such inputs in a row, then one alone) and at the edges"""
    rng = rng_for("align", fmt, ch)
    out_frames = 7001 // ch
    ins = []
    for mis, off in ((0, 0), (1, 1), (2, 2), (3, 5), (1, 4), (2, 3)):
        frames = out_frames - off - (mis % 2)
        ins.append(inp(signal(rng, fmt, frames * ch), off, vol=1.0 if mis != 2 else 0.75, mis=mis, ch=ch))
    check(be, fmt, ch, out_frames, ins, out_mis=1)
    check(be, fmt, ch, out_frames, ins[1:], out_mis=0)


# ---- 3. windows -------------------------------------------------------------------------------------------------------------------------------------
def windows(be, fmt, ch):
    rng = rng_for("windows", fmt, ch)
    out_frames = 3000
    ins = [inp(signal(rng, fmt, 37 * ch), 5, ch=ch),                    # starts and ends inside a piece
           inp(signal(rng, fmt, 1400 * ch), 100, vol=0.5, ch=ch),       # two inputs that overlap in part: 100 .. 1500 and 1000 .. 2600
           inp(signal(rng, fmt, 1600 * ch), 1000, ch=ch),
           inp(signal(rng, fmt, 8 * ch), 2700, frames=0, ch=ch),        # no frames
           inp(None, 2800, frames=100)]                                 # no data
    exp = check(be, fmt, ch, out_frames, ins)
    assert not exp[42 * ch: 100 * ch].view(np.uint8).any() and not exp[2600 * ch:].view(np.uint8).any()       # covered by no input: silence
    assert exp[:42 * ch].any() and exp[100 * ch: 2600 * ch].any()


def test_shapes(be):
    """cases 1 - 3, every format: edges on 1, 2, 3 and 6 channels, alignment and windows on 1 and 3"""
    for fmt in FORMATS:
        for ch in (1, 2, 3, 6):
            piece_and_workgroup_edges(be, fmt, ch)
        for ch in (1, 3):
            alignment(be, fmt, ch)
            windows(be, fmt, ch)


# ---- 4. the order is observable ---------------------------------------------------------------------------------------------------------------------
def order_is_observable(be, fmt):
    """+full scale, +full scale, -full scale: the saturating sum depends on the order, and the backend follows the array's"""
    top = int(np.iinfo(DT[fmt]).max)
    n, ch = 600, 2
    levels = [top, top, -top]
    outs = []
    for order in (levels, levels[::-1]):
        ins = [inp(np.full(n * ch, v, DT[fmt]), 0, ch=ch) for v in order]
        outs.append(check(be, fmt, ch, n, ins))
    assert (outs[0] == 0).all() and (outs[1] == top).all()


# ---- 5. volume ----------------------------------------------------------------------------------------------------------------------------------------
def volume(be, fmt):
    """every volume path: unity, a fraction, one that truncates, the maximum (the product clamps), the three ways to be skipped, and 1e-40, which
    is mixed (it is not below DBL_MIN) with an integer volume of 0 and a float32 volume that flushes to 0"""
    rng = rng_for("volume", fmt)
    n, ch = 700, 2
    ins = []
    for vol, mute in ((1.0, False), (0.5, False), (0.999, False), (10.0, False), (0.0, False), (DBL_MIN / 2, False), (1e-40, False), (0.5, True)):
        data = signal(rng, fmt, n * ch)
        if fmt in ("S16LE", "S32LE"):                   # full scale in a third of the samples, either sign
            info = np.iinfo(DT[fmt])
            pick = rng.integers(0, 6, n * ch)
            data = np.where(pick == 0, info.max, np.where(pick == 1, info.min, data)).astype(DT[fmt])
        ins.append(inp(data, 0, vol=vol, mute=mute, ch=ch))
    exp = check(be, fmt, ch, n, ins)
    assert be.record() == [1, 5, 3]
    if fmt in ("S16LE", "S32LE"):
        info = np.iinfo(DT[fmt])
        shift = 11 if fmt == "S16LE" else 27
        prod = (ins[3]["data"].astype(np.int64) * int(10.0 * (1 << shift))) >> shift
        assert (prod > info.max).any() and (prod < info.min).any()              # the product clamp fires
        assert (exp == info.max).any() and (exp == info.min).any()              # and the sum clamp


# ---- 6. floats ------------------------------------------------------------------------------------------------------------------------------------------
def floats(be, fmt):
    """denormals, -0.0, normal values whose sum or product is denormal, large values of both signs; no NaN"""
    dt = DT[fmt]
    tiny = np.finfo(dt).tiny                            # the smallest normal value
    big = dt(np.finfo(dt).max) / dt(4)
    special = np.array([0.0, -0.0, tiny, -tiny, tiny * dt(1.5), -tiny * dt(1.5), tiny / dt(2), -tiny / dt(4), tiny * dt(2), np.nextafter(dt(0), dt(1)),
                        big, -big, 1.0, -1.0, 3.25e-3, tiny * dt(3)], dt)
    rng = rng_for("floats", fmt)
    n, ch = 1500, 2
    ins = [inp(special[rng.integers(0, special.size, n * ch)], 0, vol=v, ch=ch) for v in (1.0, 0.5, 1.0, 0.25)]
    ins[2]["data"][: special.size * special.size] = np.repeat(special, special.size)       # every pair of special values meets
    ins[0]["data"][: special.size * special.size] = np.tile(special, special.size)
    ins[1]["data"][: special.size * special.size] = 0
    exp = check(be, fmt, ch, n, ins)
    assert not np.isnan(exp).any()
    m = model(fmt, ch, n, ins[:1])                      # the model itself flushes: one input alone comes out without its denormals
    assert (np.abs(m[m != 0]) >= tiny).all() and (np.abs(ins[0]["data"][ins[0]["data"] != 0]) < tiny).any()


def test_arithmetic(be):
    """cases 4 - 6: the order on S16 and S32, the volumes on every format, the float values on F32 and F64"""
    for fmt in ("S16LE", "S32LE"):
        order_is_observable(be, fmt)
    for fmt in FORMATS:
        volume(be, fmt)
    for fmt in ("F32LE", "F64LE"):
        floats(be, fmt)


# ---- 7. input counts ------------------------------------------------------------------------------------------------------------------------------------
def input_counts(be, fmt):
    """64 live inputs per launch; further launches start from the output of the one before, whole pieces and edge pieces alike"""
    rng = rng_for("counts", fmt)
    ch, out_frames = 2, 1700
    for n, launches in ((0, 1), (1, 1), (2, 1), (64, 1), (65, 2), (130, 3)):
        ins = []
        for k in range(n):
            off = 0 if k % 5 else int(rng.integers(0, 40))
            frames = out_frames - off - (0 if k % 7 else int(rng.integers(0, 300)))
            ins.append(inp(signal(rng, fmt, frames * ch, loud=False), off, vol=1.0 if k % 3 else 0.8, ch=ch))
        check(be, fmt, ch, out_frames, ins, out_mis=1 if n in (2, 65) else 0, launches=launches)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def refusals(be):
    rng = rng_for("refusals")
    ch, n = 2, 64
    data = signal(rng, "S16LE", n * ch)
    sc = Scene(be, "S16LE", ch, n, [inp(data, 0, ch=ch), inp(data, 0, ch=ch)])
    S16 = A.AFMT["S16LE"]

    def refused(code, fmt=S16, channels=ch, count=2, out=sc.out, out_frames=n, **change):
        arr = A.mixer_inputs(sc.inputs)
        for k, v in change.items():
            setattr(arr[1], k, v)
        assert be.mix_raw(fmt, channels, arr, count, out, out_frames) == code, (fmt, channels, count, out_frames, change)
        assert be.record() == [0, 0, 0]
        assert (sc.read() == GUARD).all()               # nothing launched: the fill is still there

    for name in ("S8", "U8", "U16LE", "U32LE"):         # the reference mixes these; not built here
        refused(ERR_UNSUPPORTED, fmt=A.AFMT[name])
    refused(ERR_INVALID, count=-1)
    refused(ERR_INVALID, out=None)
    refused(ERR_INVALID, out=sc.out + 1)
    refused(ERR_INVALID, data=sc.inputs[1].data + 1)
    refused(ERR_INVALID, out_offset=1)                  # 1 + 64 > 64
    refused(ERR_INVALID, frames=n + 1)
    refused(ERR_INVALID, out_offset=n + 1, frames=0)
    refused(ERR_INVALID, out_offset=(1 << 64) - 1, frames=2)       # the sum wraps
    refused(ERR_INVALID, out_frames=1 << 30)
    refused(ERR_INVALID, channels=0)
    refused(ERR_INVALID, channels=65)
    refused(ERR_INVALID, volume=float("nan"))
    refused(ERR_INVALID, volume=-0.5)
    refused(ERR_INVALID, volume=10.5)
    refused(ERR_INVALID, volume=float("nan"), mute=1)   # a skipped input is checked like any other
    assert sc.run().tobytes() == model("S16LE", ch, n, sc.ins).tobytes()        # and the same scene is accepted as it stands
    assert be.record() == [1, 2, 0]


def test_input_counts_and_refusals(be):
    """cases 7 and 8"""
    for fmt in ("S16LE", "F32LE"):
        input_counts(be, fmt)
    refusals(be)


# ---- 9. emulator and device agree ------------------------------------------------------------------------------------------------------------------------
def mixed_scene(fmt):
    rng = rng_for("agree", fmt)
    ch, out_frames = 3, 2500
    ins = []
    for k in range(20):
        off = int(rng.integers(0, out_frames - 1))
        frames = int(rng.integers(1, out_frames - off + 1))
        if k % 4 == 0:
            off, frames = int(rng.integers(0, 8)), out_frames - 8
        vol = (1.0, 0.3, 2.5, 0.999, 10.0)[k % 5]
        ins.append(inp(signal(rng, fmt, frames * ch, loud=k % 2 == 0), off, vol=vol, mute=k == 11, mis=k % 4, ch=ch))
    return ch, out_frames, ins


@pytest.mark.gpu
def test_emulator_and_device_agree(native_lib, emu_lib, gpu):
    for fmt in ("F32LE", "S32LE"):
        ch, out_frames, ins = mixed_scene(fmt)
        outs = [Scene(b, fmt, ch, out_frames, ins, out_mis=1).run().tobytes() for b in (Emu(emu_lib), Dev(gpu))]
        assert outs[0] == outs[1], fmt
        assert outs[0] == model(fmt, ch, out_frames, ins).tobytes(), fmt


# ---- 10. after the batched converter ------------------------------------------------------------------------------------------------------------------------
def after_convert_many(be, emu_lib):
    """four equal converters, S16 stereo 44100 -> F32 stereo 48000, through convert_many and then the mixer on the same stream with nothing in
    between; expected: the model over the outputs of four such converters run one by one"""
    plan = M.Plan("S16LE", "F32LE", in_ch=2, in_rate=44100, out_rate=48000)
    cb = M.EmuMany(emu_lib) if be.name == "emu" else M.GpuMany(be.dev)
    rng = rng_for("after")
    n_in, ch, vols = 1024, 2, (1.0, 0.5, 1.0, 0.25)
    srcs = [signal(rng, "S16LE", n_in * ch, loud=False) for _ in vols]

    def converters():
        cs = [cb.new(plan) for _ in vols]
        return cs, cb.out_frames(cs[0], n_in)

    def buffers(n_out):
        ups = [cb.upload(s.view(np.uint8)) for s in srcs]
        dsts = [cb.upload(np.full(n_out * ch * 4, GUARD, np.uint8)) for _ in vols]
        return ups, dsts

    cs, n_out = converters()                            # one by one: what the mixer is to be given
    assert 0 < n_out < 2048
    ups, dsts = buffers(n_out)
    for c, u, d in zip(cs, ups, dsts):
        assert cb.single(c, u[1], n_in, d[1], n_out) == 0
    singles = [cb.download(d[0]).view(np.float32) for d in dsts]
    for c in cs:
        cb.free(c)
    exp = model("F32LE", ch, n_out, [inp(s, 0, vol=v, ch=ch) for s, v in zip(singles, vols)])

    cs, n_out2 = converters()
    assert n_out2 == n_out
    ups, dsts = buffers(n_out)
    out = be.upload(np.full(n_out * ch * 4, GUARD, np.uint8))
    inputs = [A.MixerInput(d[1], 0, n_out, v, 0, 0) for d, v in zip(dsts, vols)]
    if be.name == "emu":
        assert cb.many(cs, [u[1] for u in ups], [n_in] * 4, [d[1] for d in dsts], [n_out] * 4) == 0
        assert be.mix("F32LE", ch, inputs, out[1], n_out) == OK
    else:
        import torch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())  # the uploads above
        A.convert_many(cs, [u[1] for u in ups], [n_in] * 4, [d[1] for d in dsts], [n_out] * 4, stream=side.cuda_stream)
        assert be.mix("F32LE", ch, inputs, out[1], n_out, stream=side.cuda_stream) == OK
        side.synchronize()
    assert cb.debug()[:2] == [1, 4]                    # the four went as one batched run
    assert be.record() == [1, 4, 0]
    assert be.download(out[0]).tobytes() == exp.tobytes()
    for c in cs:
        cb.free(c)


def test_scenes(be, emu_lib):
    """the scene of case 9 against the model on each backend, and case 10"""
    for fmt in ("F32LE", "S32LE"):
        ch, out_frames, ins = mixed_scene(fmt)
        check(be, fmt, ch, out_frames, ins, out_mis=1)
    after_convert_many(be, emu_lib)
