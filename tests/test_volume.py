"""volume: fixed and per-frame gains on six formats, many buffers a launch - gstamd_audio_volume_process / _process_many / k_audio_volume
(DESIGN 3.10).

Nothing here needs the reference tree.  The expected bytes of every case come from tests/volume_model.py: a numpy restatement of the two
tables of DESIGN 3.10.1, which imports nothing from gstreamer_amd/csrc and does not call the emulator.  Outputs are compared as bytes, with
no tolerance.  The record of every call (launches, buffers scaled, passed through, silenced) is checked with the bytes.

1. piece and workgroup edges;  2. alignment of `out` and `in`;  3. the fixed-volume rules;  4. the gains rules;  5. many buffers;
6. refusals;  7. emulator and device agree (GPU only);  8. behind the batched converter and in front of the mixer on one stream;  9. the
model against the stock `volume` element (CPU only; the one test that may skip).

Cases 1 - 6 and 8 run twice: -m "not gpu" on the host emulator (tests/emu/emu_audio_volume.cpp walks the grid lane by lane with the library's
launch plan), -m gpu through the C ABI on the device.  Every buffer and gains array of a call sits inside one allocation between guard
bytes; out-of-place outputs are pre-filled with the guard pattern, and after the call every byte outside the outputs - inputs and gains
included - must be what it was."""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from gstreamer_amd import audio as A
import volume_model as VM
import test_audio_convert_many as M
import test_audio_mixer as MX

GUARD, GUARD_BYTES = 0xA5, 64
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2        # include/gstamd_video.h; checked against the binding in the GPU tests
FORMATS = VM.FORMATS
# the settings the rules of (a) were checked with against the stock element, and one whose float is 0
SETTINGS = [(1.0, False), (0.5, False), (0.999, False), (0.7, False), (1.3, False), (10.0, False), (0.0, False), (1e-3, False), (1.0004, False),
            (1.0006, False), (0.3333, False), (9.99, False), (1e-5, False), (0.7, True), (1e-46, False)]
RAMPS = [(0.0, 1.0), (1.3, 0.2), (10.0, 9.0), (1.0, 1.0), (0.0, 0.0)]
HERE = os.path.dirname(os.path.abspath(__file__))


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def ramp(g0, g1, frames):
    return g0 + (g1 - g0) * np.arange(frames, dtype=np.float64) / float(max(frames, 1))


def signal(rng, fmt, n):
    """integers over the full range, floats around +-1"""
    if fmt in VM.BITS:
        bits = VM.BITS[fmt]
        return rng.integers(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, n, dtype=np.int64, endpoint=True).astype(VM.DT[fmt])
    return rng.standard_normal(n).astype(VM.DT[fmt])


# ---- backends ---------------------------------------------------------------------------------------------------------------------------------
class Emu:
    """tests/emu/emu_audio_volume.cpp"""
    name = "emu"

    def __init__(self, emu):
        self.e = emu
        emu.emu_audio_volume_process_many.argtypes = [C.c_int, C.c_int, C.POINTER(A.VolumeBuffer), C.c_int, C.c_void_p]
        emu.emu_audio_volume_debug_launches.argtypes = [C.POINTER(C.c_int32), C.c_int]

    def upload(self, host):
        a = np.zeros(host.size + 64, np.uint8)
        o = (-a.ctypes.data) % 64
        a[o: o + host.size] = host
        return (a, o, host.size), a.ctypes.data + o

    def download(self, keep):
        a, o, n = keep
        return a[o: o + n].copy()

    def many_raw(self, fmt, ch, arr, n, stream=None):
        """the status; a refusal needs no text here (the emulator runs the library's plan, not its entry point)"""
        return self.e.emu_audio_volume_process_many(fmt, ch, arr, n, None)

    def single(self, fmt, ch, b, stream=None):
        return self.many_raw(A.AFMT[fmt], ch, A.volume_buffers([b]), 1)

    def record(self):
        buf = (C.c_int32 * 4)()
        assert self.e.emu_audio_volume_debug_launches(buf, 4) == 4
        return list(buf)


class Dev:
    """k_audio_volume through the C ABI and its Python mirror"""
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

    def many_raw(self, fmt, ch, arr, n, stream=None):
        from gstreamer_amd import video as V
        status = A._vol_lib().gstamd_audio_volume_process_many(fmt, ch, arr, n, stream)
        assert status == OK or V.last_error()           # a refusal leaves its text in gstamd_last_error
        return status

    def single(self, fmt, ch, b, stream=None):
        from gstreamer_amd import video as V
        try:
            A.volume_process(fmt, ch, b.in_, b.out, b.frames, b.volume, b.mute, b.gains, stream)
        except V.GstAmdError as e:
            assert str(e)
            return e.code
        return OK

    def record(self):
        d = A.volume_debug()
        return [d["launches"], d["scaled"], d["passed"], d["silenced"]]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request, native_lib, emu_lib):
    return Emu(emu_lib) if request.param == "emu" else Dev(request.getfixturevalue("gpu"))


# ---- one call: every buffer and gains array inside one allocation, between guard bytes ----------------------------------------------------------
def buf(data, volume=1.0, mute=False, gains=None, oop=False, in_mis=0, out_mis=0):
    """one buffer: data a flat sample array of VM.DT; oop: out of place; in_mis / out_mis: BYTES the pointer sits past a 16-byte boundary (in
    place: in_mis counts)"""
    return {"data": data, "volume": volume, "mute": mute, "gains": gains, "oop": oop, "in_mis": in_mis, "out_mis": out_mis}


def kind_of(b):
    """'scaled' (rule (a)'s formulas, or gains), 'pass' or 'silence'"""
    if b["gains"] is not None:
        return "scaled"
    return {"scale": "scaled", "pass": "pass", "silence": "silence"}[VM.fixed_kind(b["volume"], b["mute"])]


def expected(fmt, ch, b):
    if b["gains"] is not None:
        return VM.to_bytes(fmt, VM.gains(fmt, ch, b["data"], b["gains"], b["mute"]))
    return VM.to_bytes(fmt, VM.fixed(fmt, b["data"], b["volume"], b["mute"]))


def expected_record(bufs):
    live = [b for b in bufs if b["data"].size]
    kernel = sum(1 for b in live if not (kind_of(b) == "pass" and not b["oop"]))
    return [(kernel + 63) // 64] + [sum(1 for b in live if kind_of(b) == k) for k in ("scaled", "pass", "silence")]


class Scene:
    """per buffer: its input, its output when out of place (pre-filled with the guard pattern), its gains; every block has GUARD_BYTES or more
    of guard pattern on both sides"""

    def __init__(self, be, fmt, ch, bufs):
        self.be, self.fmt, self.ch, self.bufs = be, fmt, ch, bufs
        bps = VM.BPS[fmt]
        pos, place = 0, []

        def block(size, mis):
            nonlocal pos
            pos = (pos + GUARD_BYTES + 63) // 64 * 64 + mis
            at = pos
            pos += size
            return at

        for b in bufs:
            size = b["data"].size * bps
            i = block(size, b["in_mis"])
            o = block(size, b["out_mis"]) if b["oop"] else i
            g = None if b["gains"] is None else block(b["gains"].size * 8, 0)
            place.append((i, o, g, size))
        self.place = place
        self.image = np.full(pos + GUARD_BYTES, GUARD, np.uint8)
        for b, (i, o, g, size) in zip(bufs, place):
            self.image[i: i + size] = VM.to_bytes(fmt, b["data"])
            if g is not None:
                self.image[g: g + b["gains"].size * 8] = np.ascontiguousarray(b["gains"], np.float64).view(np.uint8)
        self.keep, self.base = be.upload(self.image)
        assert self.base % 64 == 0
        self.buffers = [A.VolumeBuffer(self.base + i, self.base + o, b["data"].size // ch, b["volume"], None if g is None else self.base + g,
                                       int(b["mute"]), 0) for b, (i, o, g, size) in zip(bufs, place)]

    def read(self):
        """every buffer's output bytes, after checking that nothing else changed: the guards, the inputs of out-of-place buffers, the gains"""
        got = self.be.download(self.keep)
        outside = np.ones(got.size, bool)
        for _, o, _, size in self.place:
            outside[o: o + size] = False
        assert (got[outside] == self.image[outside]).all(), "bytes outside the outputs changed"
        return [got[o: o + size] for _, o, _, size in self.place]

    def run(self, stream=None):
        assert self.be.many_raw(A.AFMT[self.fmt], self.ch, A.volume_buffers(self.buffers), len(self.buffers), stream) == OK
        return self.read()

    def run_singles(self):
        for b in self.buffers:
            assert self.be.single(self.fmt, self.ch, b) == OK
        return self.read()


def check(be, fmt, ch, bufs):
    """run one scene; bytes against the model, the record against the buffers"""
    outs = Scene(be, fmt, ch, bufs).run()
    assert be.record() == expected_record(bufs), (be.name, fmt, ch)
    for k, (b, got) in enumerate(zip(bufs, outs)):
        exp = expected(fmt, ch, b)
        assert got.tobytes() == exp.tobytes(), (be.name, fmt, ch, k, b["data"].size, b["volume"], b["mute"], b["oop"], b["in_mis"], b["out_mis"],
                                                int(np.argmax(got != exp)))
    return outs


# ---- 1. piece and workgroup edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_piece_and_workgroup_edges(be, fmt):
    """volume 0.7, in place and out of place, sample counts around a piece, a workgroup and two; with 3 channels the counts as frames (a frame
    never lines up with a piece) and as the samples they are nearest to"""
    P = VM.PIECE[fmt]
    rng = rng_for("edges", fmt)
    for count in (1, 3, P - 1, P, P + 1, 256 * P - 1, 256 * P, 256 * P + 1, 512 * P + 5):
        for ch, frames in ((1, count), (3, count), (3, (count + 2) // 3)):
            data = signal(rng, fmt, frames * ch)
            check(be, fmt, ch, [buf(data, 0.7), buf(data, 0.7, oop=True)])


# ---- 2. alignment ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_alignment(be, fmt):
    """`out` 0 .. 3 samples past a 16-byte boundary, `in` 0 .. 3 samples past one and 4 and 8 bytes past one (every load width of the format);
    S24: every byte offset 0 .. 3 of both; out of place, and in place at each offset; long enough for workgroups of whole pieces"""
    P, bps = VM.PIECE[fmt], VM.BPS[fmt]
    rng = rng_for("align", fmt)
    n = 600 * P + 7
    if fmt == "S24LE":
        outs, ins = [0, 1, 2, 3], [0, 1, 2, 3]
    else:
        outs = [k * bps for k in range(4)]
        ins = sorted(set(outs) | {o for o in (4, 8) if o % bps == 0})
    bufs = [buf(signal(rng, fmt, n), 0.7, oop=True, in_mis=i, out_mis=o) for o in outs for i in ins]
    bufs += [buf(signal(rng, fmt, n), 0.7, in_mis=o) for o in outs]
    check(be, fmt, 1, bufs)
    g = ramp(1.3, 0.2, n // 3)                          # and the gains path at each output offset, the frame walk starting inside a frame
    check(be, fmt, 3, [buf(signal(rng, fmt, n // 3 * 3), gains=g, oop=k % 2 == 0, in_mis=ins[-1 - k], out_mis=o) for k, o in enumerate(outs)])


# ---- 3. the fixed-volume rules ----------------------------------------------------------------------------------------------------------------------
def fixed_input(fmt, rng, nan=False):
    if fmt == "S8":
        return np.arange(-128, 128).astype(np.int8)                     # all 256 values
    if fmt == "S16LE":
        return np.arange(-32768, 32768).astype(np.int16)                # all 65,536 values
    if fmt in VM.BITS:
        top = (1 << (VM.BITS[fmt] - 1)) - 1
        return np.concatenate([np.array([top, -top - 1, top - 1, -top, 1, -1, 0], np.int32), signal(rng, fmt, 4096)])
    dt = VM.DT[fmt]
    tiny, big = np.finfo(dt).tiny, dt(np.finfo(dt).max) / dt(4)
    special = [0.0, -0.0, tiny / dt(2), -tiny / dt(4), np.nextafter(dt(0), dt(1)), tiny, -tiny, tiny * dt(1.25), -tiny * dt(1.4), tiny * dt(3),
               big, -big, np.inf, -np.inf, 1.0, -1.0] + ([np.nan] if nan else [])
    return np.concatenate([np.array(special, dt), rng.standard_normal(4096).astype(dt)])


@pytest.mark.parametrize("fmt", FORMATS)
def test_fixed_volume_rules(be, fmt):
    """the 15 settings as the 15 buffers of one call, alternately in place and out of place (a NaN among the floats that are silenced or
    passed through: NaN payloads of products are not pinned)"""
    rng = rng_for("fixed", fmt)
    bufs = [buf(fixed_input(fmt, rng, nan=VM.fixed_kind(v, m) != "scale"), v, m, oop=k % 2 == 1) for k, (v, m) in enumerate(SETTINGS)]
    outs = check(be, fmt, 1, bufs)
    assert be.record() == [1, 10, 2, 3]                 # 1.0 and 1.0004 pass; 0.0, 1e-46 and the muted one are silenced
    by = {s: (b, o) for s, b, o in zip(SETTINGS, bufs, outs)}
    data = by[(0.7, False)][0]["data"]
    if fmt in ("S32LE", "F64LE"):                       # the float-held volume is observable: the double 0.7 gives other bytes
        wrong = VM.to_bytes(fmt, VM.fixed(fmt, data, 0.7, as_type=np.float64))
        assert wrong.tobytes() != by[(0.7, False)][1].tobytes()
    for setting in ((1.0004, False), (1.0, False)):     # the input's bytes, denormals (and the NaN) among them
        b, o = by[setting]
        assert o.tobytes() == VM.to_bytes(fmt, b["data"]).tobytes()
    assert VM.fixed_kind(1.0006, False) == "scale" and VM.fixed_kind(1e-46, False) == "silence" and VM.fixed_kind(1e-5, False) == "scale"
    if fmt in ("F32LE", "F64LE"):
        dt = VM.DT[fmt]
        d = by[(1.0004, False)][0]["data"]
        assert ((d != 0) & (np.abs(d) < np.finfo(dt).tiny)).any() and np.isnan(d).any()
        muted = by[(0.7, True)]
        assert np.signbit(muted[0]["data"][1]) and muted[0]["data"][1] == 0 and not muted[1].any()      # mute on -0.0: zero bytes
        scaled = VM.from_bytes(fmt, by[(0.7, False)][1])                # the scaling rows flush: no denormal comes out
        assert (np.abs(scaled[scaled != 0]) >= np.finfo(dt).tiny).all() and np.isinf(VM.from_bytes(fmt, by[(10.0, False)][1])).sum() >= 4


# ---- 4. the gains rules -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_gains_rules(be, fmt):
    """channels 1, 2, 3, 6 x five ramps x frames 1, 255, 1027: the 15 buffers of a channel count in one call"""
    for ch in (1, 2, 3, 6):
        rng = rng_for("gains", fmt, ch)
        bufs = [buf(signal(rng, fmt, frames * ch), gains=ramp(g0, g1, frames), oop=(k + frames) % 2 == 0)
                for k, (g0, g1) in enumerate(RAMPS) for frames in (1, 255, 1027)]
        check(be, fmt, ch, bufs)
        assert be.record() == [1, 15, 0, 0]             # no passthrough and no silence shortcut: g = 1.0 and g = 0.0 go through the formulas


def test_gains_channel_switch(be):
    """S16 with all 65,536 values at 2 and at 3 channels, and F32 at 3: the reference's ORC rows and its C rows give different bytes, so the
    channel count at which the kernel switches is observable; mute with gains"""
    all16 = np.arange(-32768, 32768).astype(np.int16)
    for ch, data in ((2, all16), (3, np.concatenate([all16, all16[:2]]))):
        for g0, g1 in ((1.3, 0.2), (10.0, 9.0)):
            check(be, "S16LE", ch, [buf(data, gains=ramp(g0, g1, data.size // ch))])
    data = np.concatenate([all16, all16[:2]])
    g = ramp(1.3, 0.2, data.size // 3)
    assert (VM.gains("S16LE", 3, data, g, doubles=False) != VM.gains("S16LE", 3, data, g, doubles=True)).any()
    rng = rng_for("switch")
    f = signal(rng, "F32LE", 3 * 1027)
    g = ramp(1.3, 0.2, 1027)
    assert (VM.gains("F32LE", 3, f, g, doubles=False) != VM.gains("F32LE", 3, f, g, doubles=True)).any()
    for ch in (2, 3):                                   # the same samples on either side of the switch
        part = f[: f.size // ch * ch]
        check(be, "F32LE", ch, [buf(part, gains=ramp(1.3, 0.2, part.size // ch))])
    ones = np.full(6, -1.0, np.float32)                 # mute: every gain is +0.0 and the formulas still run
    for ch in (1, 3):
        out = check(be, "F32LE", ch, [buf(ones, gains=np.full(6 // ch, 0.5), mute=True)])[0]
        assert (out.view(np.uint32) == 0x80000000).all()


def test_gains_denormals(be):
    """denormal inputs and denormal products: kept on the two plain-IEEE rows (F32 at 3 channels and more, F64 at 2 and more), flushed on their
    counterparts (F32 at 1 and 2, F64 at 1)"""
    for fmt, plain_ch, flushed_ch in (("F32LE", 3, 2), ("F64LE", 2, 1)):
        dt = VM.DT[fmt]
        tiny = np.finfo(dt).tiny
        base = np.array([tiny / dt(2), -tiny / dt(8), np.nextafter(dt(0), dt(1)), tiny, -tiny * dt(1.5), tiny * dt(3), 1.0, -1.0, 0.0, -0.0, tiny * dt(100),
                         -tiny * dt(1000)], dt)
        frames = 6 * 41
        data = {ch: np.tile(base, frames * ch // base.size + 1)[: frames * ch] for ch in (1, 2, 3, 6)}
        g = np.tile(np.array([1.0, 0.5, 1e-3, 0.75, 2.0, 1e-2]), frames // 6)          # denormal x 1.0, normal x 1e-3 -> denormal, ...
        outs = {ch: VM.from_bytes(fmt, check(be, fmt, ch, [buf(data[ch], gains=g, oop=ch % 2 == 0)])[0]) for ch in (1, 2, 3, 6)}
        for ch, out in outs.items():
            sub = (out != 0) & (np.abs(out) < tiny)
            assert sub.any() == VM.uses_doubles(fmt, ch), (fmt, ch)
        # the same samples and gains in the flushed row: a zero where the plain row has a denormal
        one = data[flushed_ch][: frames]
        plain = VM.gains(fmt, plain_ch, np.repeat(one, plain_ch), g)[::plain_ch]
        flushed = VM.gains(fmt, flushed_ch, np.repeat(one, flushed_ch), g)[::flushed_ch]
        assert (((plain != 0) & (np.abs(plain) < tiny)) & (flushed == 0)).any()
    # F64 at 2 channels returns a denormal where F64 at 1 channel returns a zero: the same frames, through the backend
    tiny = np.finfo(np.float64).tiny
    mono = np.array([tiny * 3, 1.0, tiny / 2, -tiny], np.float64)
    g = np.array([0.25, 1.0, 1.0, 0.5])
    o1 = VM.from_bytes("F64LE", check(be, "F64LE", 1, [buf(mono, gains=g)])[0])
    o2 = VM.from_bytes("F64LE", check(be, "F64LE", 2, [buf(np.repeat(mono, 2), gains=g)])[0])[::2]
    assert o1[0] == 0 and o2[0] == tiny * 0.75 and o1[2] == 0 and o2[2] == tiny / 2 and o1[1] == o2[1] == 1.0


# ---- 5. many buffers -----------------------------------------------------------------------------------------------------------------------------------
def many_scene(fmt, ch, n, rng):
    """n buffers of all kinds and of lengths around the piece and workgroup edges"""
    P = VM.PIECE[fmt]
    lengths = (1, P - 1, P, P + 1, 256 * P + 1, 3 * P + 2, 40 * P, 256 * P - 1)
    bufs = []
    for k in range(n):
        frames = (lengths[k % len(lengths)] + ch - 1) // ch
        data = signal(rng, fmt, frames * ch)
        kind = k % 5
        if kind == 0:
            bufs.append(buf(data, 0.7, oop=k % 2 == 0, out_mis=VM.BPS[fmt] * (k % 3)))
        elif kind == 1:
            bufs.append(buf(data, gains=ramp(1.3, 0.2, frames), oop=k % 2 == 1))
        elif kind == 2:
            bufs.append(buf(data, 0.0 if k % 2 else 0.5, mute=k % 2 == 0, oop=k % 4 < 2))
        elif kind == 3:
            bufs.append(buf(data, 1.0))                 # passthrough in place: in no launch
        else:
            bufs.append(buf(data, 1.0004, oop=True))    # passthrough out of place: a copy
    return bufs


def kernel_only(fmt, ch, n, rng):
    """n buffers that all need the kernel"""
    return [b for b in many_scene(fmt, ch, 2 * n, rng) if not (kind_of(b) == "pass" and not b["oop"])][:n]


@pytest.mark.parametrize("fmt", ["S16LE", "S24LE", "F32LE"])
def test_many_buffers(be, fmt):
    rng = rng_for("many", fmt)
    ch = 2
    assert be.many_raw(A.AFMT[fmt], ch, None, 0) == OK and be.record() == [0, 0, 0, 0]
    for n, launches in ((1, 1), (5, 1), (64, 1), (65, 2), (130, 3)):
        bufs = many_scene(fmt, ch, n, rng) if n == 5 else kernel_only(fmt, ch, n, rng)
        outs = check(be, fmt, ch, bufs)
        assert be.record()[0] == launches
        singles = Scene(be, fmt, ch, bufs).run_singles()        # and what n single calls give
        assert [o.tobytes() for o in outs] == [o.tobytes() for o in singles]
    bufs = many_scene(fmt, ch, 5, rng)
    assert [kind_of(b) for b in bufs] == ["scaled", "scaled", "silence", "pass", "pass"] and bufs[1]["gains"] is not None
    assert [b["oop"] for b in bufs[3:]] == [False, True]        # the five of n = 5: one of each kind
    mixed = many_scene(fmt, ch, 150, rng)               # with in-place passthrough in between: 120 descriptors, 2 launches
    check(be, fmt, ch, mixed)
    assert be.record() == [2, 60, 60, 30]
    quiet = [buf(signal(rng, fmt, 300 * ch), v) for v in (1.0, 1.0004, 1.0)] + [buf(signal(rng, fmt, 0), 0.5), buf(signal(rng, fmt, 0), 0.0, oop=True)]
    check(be, fmt, ch, quiet)                           # in-place passthrough and empty buffers only: nothing launched, nothing written
    assert be.record() == [0, 0, 3, 0]


def test_past_the_grid_cap(be):
    """a buffer with more pieces than 2048 workgroups x 256 lanes: the grid-stride walk, next to a short buffer whose workgroups exit at once"""
    rng = rng_for("cap")
    n = (2048 * 256 + 2 * 256 + 3) * VM.PIECE["S16LE"] + 5
    check(be, "S16LE", 1, [buf(signal(rng, "S16LE", n), 0.7, in_mis=2), buf(signal(rng, "S16LE", 77), gains=ramp(0.0, 1.0, 77), oop=True)])
    assert be.record() == [1, 2, 0, 0]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(be):
    rng = rng_for("refusals")
    ch, n = 2, 64
    data = signal(rng, "S16LE", n * ch)
    sc = Scene(be, "S16LE", ch, [buf(data, 0.5, oop=True), buf(data, 0.5, oop=True), buf(data, gains=ramp(0.0, 1.0, n), oop=True)])
    S16 = A.AFMT["S16LE"]
    size = n * ch * 2

    def refused(code, fmt=S16, channels=ch, count=3, null=False, which=1, **change):
        arr = A.volume_buffers(sc.buffers)
        for k, v in change.items():
            setattr(arr[which], k, v)
        assert be.many_raw(fmt, channels, None if null else arr, count) == code, (fmt, channels, count, change)
        assert be.record() == [0, 0, 0, 0]
        assert all((o == GUARD).all() for o in sc.read())       # nothing launched: every output's fill is still there

    for name in ("U8", "S16BE", "S24_32LE", "F32BE"):
        refused(ERR_UNSUPPORTED, fmt=A.AFMT[name])
    refused(ERR_INVALID, channels=0)
    refused(ERR_INVALID, channels=65)
    refused(ERR_INVALID, frames=1 << 30)
    refused(ERR_INVALID, in_=None)
    refused(ERR_INVALID, out=None)
    refused(ERR_INVALID, in_=sc.buffers[1].in_ + 1)
    refused(ERR_INVALID, out=sc.buffers[1].out + 1)
    refused(ERR_INVALID, which=2, gains=sc.buffers[2].gains + 4)
    refused(ERR_INVALID, out=sc.buffers[1].in_ + 2)                     # overlapping without being equal, either way round
    refused(ERR_INVALID, out=sc.buffers[1].in_ - 2)
    refused(ERR_INVALID, out=sc.buffers[1].in_ + size - 2)
    refused(ERR_INVALID, volume=float("nan"))
    refused(ERR_INVALID, volume=-0.5)
    refused(ERR_INVALID, volume=10.5)
    refused(ERR_INVALID, volume=float("nan"), mute=1)
    refused(ERR_INVALID, count=-1)
    refused(ERR_INVALID, null=True)
    arr = A.volume_buffers(sc.buffers)                  # the volume of a buffer with gains is ignored; the same scene is accepted as it stands
    arr[2].volume = float("nan")
    assert be.many_raw(S16, ch, arr, 3) == OK and be.record() == [1, 3, 0, 0]
    assert [o.tobytes() for o in sc.read()] == [expected("S16LE", ch, b).tobytes() for b in sc.bufs]
    sc24 = Scene(be, "S24LE", 1, [buf(signal(rng, "S24LE", 40), 0.5, oop=True, in_mis=1, out_mis=3)])          # S24: any byte address
    assert sc24.run()[0].tobytes() == expected("S24LE", 1, sc24.bufs[0]).tobytes()


# ---- 7. emulator and device agree -----------------------------------------------------------------------------------------------------------------------------
def mixed_scene(fmt, ch):
    rng = rng_for("agree", fmt)
    P, bps = VM.PIECE[fmt], VM.BPS[fmt]
    bufs = []
    for k in range(20):
        frames = int(rng.integers(1, 700 * P)) // ch + 1
        data = signal(rng, fmt, frames * ch)
        mis = dict(in_mis=int(rng.integers(0, 4)) * (1 if fmt == "S24LE" else bps), out_mis=int(rng.integers(0, 4)) * (1 if fmt == "S24LE" else bps))
        oop = bool(rng.integers(0, 2))
        if k % 4 == 0:
            bufs.append(buf(data, gains=ramp(*RAMPS[k % 5], frames), mute=k == 8, oop=oop, **mis))
        else:
            v, m = SETTINGS[(3 * k) % len(SETTINGS)]
            bufs.append(buf(data, v, m, oop=oop, **mis))
    return bufs


@pytest.mark.gpu
def test_emulator_and_device_agree(native_lib, emu_lib, gpu):
    for fmt, ch in (("F32LE", 3), ("S24LE", 2), ("S8", 1)):
        bufs = mixed_scene(fmt, ch)
        outs = [[o.tobytes() for o in Scene(b, fmt, ch, bufs).run()] for b in (Emu(emu_lib), Dev(gpu))]
        assert outs[0] == outs[1], fmt
        assert outs[0] == [expected(fmt, ch, b).tobytes() for b in bufs], fmt


def test_mixed_scene(be):
    """the scenes of case 7 against the model on each backend"""
    for fmt, ch in (("F32LE", 3), ("S24LE", 2), ("S8", 1)):
        check(be, fmt, ch, mixed_scene(fmt, ch))


# ---- 8. on one stream ---------------------------------------------------------------------------------------------------------------------------------------------
def test_between_converter_and_mixer(be, emu_lib):
    """four equal converters, S16 stereo 44100 -> F32 stereo 48000, through convert_many, the volumes in place on their outputs - a fixed
    volume, gains, a mute, a passthrough - and the mixer, on one stream with nothing in between; expected: converter output -> the volume
    model -> the mixer test's model"""
    plan = M.Plan("S16LE", "F32LE", in_ch=2, in_rate=44100, out_rate=48000)
    cb = M.EmuMany(emu_lib) if be.name == "emu" else M.GpuMany(be.dev)
    mx = MX.Emu(emu_lib) if be.name == "emu" else MX.Dev(be.dev)
    rng = rng_for("stream")
    n_in, ch = 1024, 2
    srcs = [MX.signal(rng, "S16LE", n_in * ch, loud=False) for _ in range(4)]

    def converters():
        cs = [cb.new(plan) for _ in srcs]
        return cs, cb.out_frames(cs[0], n_in)

    def buffers(n_out):
        ups = [cb.upload(s.view(np.uint8)) for s in srcs]
        dsts = [cb.upload(np.full(n_out * ch * 4, GUARD, np.uint8)) for _ in srcs]
        return ups, dsts

    cs, n_out = converters()                            # one by one: what the volumes are to be given
    assert 0 < n_out < 2048
    ups, dsts = buffers(n_out)
    for c, u, d in zip(cs, ups, dsts):
        assert cb.single(c, u[1], n_in, d[1], n_out) == 0
    singles = [cb.download(d[0]).view(np.float32) for d in dsts]
    for c in cs:
        cb.free(c)
    g = ramp(0.0, 1.0, n_out)
    scaled = [VM.fixed("F32LE", singles[0], 0.7), VM.gains("F32LE", ch, singles[1], g), VM.fixed("F32LE", singles[2], 0.5, True),
              VM.fixed("F32LE", singles[3], 1.0)]
    assert scaled[0].any() and scaled[1].any() and not scaled[2].any() and scaled[3].tobytes() == singles[3].tobytes()
    exp = MX.model("F32LE", ch, n_out, [MX.inp(s, 0, ch=ch) for s in scaled])

    cs, n_out2 = converters()
    assert n_out2 == n_out
    ups, dsts = buffers(n_out)
    gd = be.upload(g.view(np.uint8))
    out = be.upload(np.full(n_out * ch * 4, GUARD, np.uint8))
    vols = [A.VolumeBuffer(dsts[0][1], dsts[0][1], n_out, 0.7, None, 0, 0), A.VolumeBuffer(dsts[1][1], dsts[1][1], n_out, 1.0, gd[1], 0, 0),
            A.VolumeBuffer(dsts[2][1], dsts[2][1], n_out, 0.5, None, 1, 0), A.VolumeBuffer(dsts[3][1], dsts[3][1], n_out, 1.0, None, 0, 0)]
    inputs = [A.MixerInput(d[1], 0, n_out, 1.0, 0, 0) for d in dsts]
    if be.name == "emu":
        assert cb.many(cs, [u[1] for u in ups], [n_in] * 4, [d[1] for d in dsts], [n_out] * 4) == 0
        assert be.many_raw(A.AFMT["F32LE"], ch, A.volume_buffers(vols), 4) == OK
        assert mx.mix("F32LE", ch, inputs, out[1], n_out) == OK
    else:
        import torch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())  # the uploads above
        A.convert_many(cs, [u[1] for u in ups], [n_in] * 4, [d[1] for d in dsts], [n_out] * 4, stream=side.cuda_stream)
        A.volume_process_many("F32LE", ch, vols, stream=side.cuda_stream)
        assert mx.mix("F32LE", ch, inputs, out[1], n_out, stream=side.cuda_stream) == OK
        side.synchronize()
    assert cb.debug()[:2] == [1, 4]                    # the four went as one batched run
    assert be.record() == [1, 2, 1, 1]
    assert mx.record() == [1, 4, 0]
    assert be.download(out[0]).tobytes() == exp.tobytes()
    for c in cs:
        cb.free(c)


# ---- 9. the model against the stock element ---------------------------------------------------------------------------------------------------------------------------
STOCK = "/opt/conda"
PCM = {"S8": "s8", "S16LE": "s16le", "S24LE": "s24le", "S32LE": "s32le", "F32LE": "f32le", "F64LE": "f64le"}


def stock_env(tmp_path):
    launch = os.path.join(STOCK, "bin", "gst-launch-1.0")
    plugins = os.path.join(STOCK, "lib", "gstreamer-1.0")
    needed = [launch, os.path.join(STOCK, "lib", "libgstreamer-1.0.so.0"), os.path.join(STOCK, "lib", "libgstcontroller-1.0.so.0")]
    needed += [os.path.join(plugins, f) for f in ("libgstvolume.so", "libgstrawparse.so", "libgstcoreelements.so")]
    if not all(os.path.exists(p) for p in needed):
        pytest.skip("the stock GStreamer runtime and its volume plugin are not installed here")
    env = dict(os.environ)
    env["GST_PLUGIN_SYSTEM_PATH"] = plugins
    env["GST_REGISTRY"] = str(tmp_path / "registry.bin")
    return launch, env


def stock_input(fmt, rng, n=4096):
    """the extremes, +-0, denormals and the minimum normal, then draws; exactly n samples"""
    if fmt in VM.BITS:
        top = (1 << (VM.BITS[fmt] - 1)) - 1
        head = np.array([top, -top - 1, top - 1, -top, 1, -1, 0], np.int64).astype(VM.DT[fmt])
    else:
        dt = VM.DT[fmt]
        tiny = np.finfo(dt).tiny
        head = np.array([0.0, -0.0, tiny / dt(2), -tiny / dt(4), np.nextafter(dt(0), dt(1)), tiny, -tiny, tiny * dt(1.25), -tiny * dt(1.4), 1.0, -1.0,
                         np.finfo(dt).max / dt(4), -np.finfo(dt).max / dt(4)], dt)
    return np.concatenate([head, signal(rng, fmt, n - head.size)])


def test_model_against_stock_element_fixed(tmp_path):
    """rule (a) of the MODEL (never the product) against the stock 1.14 `volume` element on the CPU: 6 formats x 14 settings x 4096 mono
    samples through gst-launch-1.0, one process per format, byte for byte"""
    launch, env = stock_env(tmp_path)
    for fmt in FORMATS:
        rng = rng_for("stock", fmt)
        data = stock_input(fmt, rng)
        src = tmp_path / ("in_%s.raw" % fmt)
        VM.to_bytes(fmt, data).tofile(str(src))
        size = data.size * VM.BPS[fmt]
        args = [launch, "-q"]
        for k, (v, m) in enumerate(SETTINGS[:14]):
            args += ["filesrc", "location=%s" % src, "blocksize=%d" % size, "!", "rawaudioparse", "format=pcm", "pcm-format=%s" % PCM[fmt],
                     "sample-rate=48000", "num-channels=1", "!", "volume", "volume=%r" % v, "mute=%s" % ("true" if m else "false"), "!", "filesink",
                     "location=%s" % (tmp_path / ("out_%s_%d.raw" % (fmt, k)))]
        r = subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        if r.returncode != 0 and b"no element" in r.stdout:
            pytest.skip("the stock runtime lacks an element of the pipeline: %s" % r.stdout.decode(errors="replace")[-200:])
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
        for k, (v, m) in enumerate(SETTINGS[:14]):
            got = np.fromfile(str(tmp_path / ("out_%s_%d.raw" % (fmt, k))), np.uint8)
            exp = VM.to_bytes(fmt, VM.fixed(fmt, data, v, m))
            assert got.size == exp.size and int((got != exp).sum()) == 0, (fmt, v, m, int((got != exp).sum()) if got.size == exp.size else got.size)
    # the check discriminates: the same model with the volume held as a double gives other bytes
    data = stock_input("S32LE", rng_for("stock", "S32LE"))
    assert VM.fixed("S32LE", data, 0.7, as_type=np.float64).tobytes() != VM.fixed("S32LE", data, 0.7).tobytes()


STOCK_RAMPS = [(0.05, 0.05), (0.0, 0.1), (0.13, 0.02), (1.0, 0.9), (0.1, 0.1), (0.0, 0.0), (0.07, 0.0999)]


def test_model_against_stock_element_gains(tmp_path):
    """rule (b) of the MODEL against the stock element with a linear GstInterpolationControlSource bound to `volume`, driven from a child
    process (tests/volume_stock_child.py); the gains themselves are read back through an all-ones F64 mono buffer of the same length.  7
    ramps x 6 formats mono, and the channel rule at 1, 2, 3, 6, 8 channels; every file is one buffer of at most 64 KB"""
    _, env = stock_env(tmp_path)
    jobs, cases = [], []

    def job(fmt, ch, frames, r, data):
        k = len(jobs)
        src, dst = tmp_path / ("g_in_%d.raw" % k), tmp_path / ("g_out_%d.raw" % k)
        VM.to_bytes(fmt, data).tofile(str(src))
        assert data.size * VM.BPS[fmt] <= 65536
        jobs.append({"src": str(src), "dst": str(dst), "pcm": PCM[fmt], "channels": ch, "frames": frames, "rate": 48000, "c0": r[0], "c1": r[1]})
        return str(dst)

    for r in STOCK_RAMPS:
        for fmt, ch in [(f, 1) for f in FORMATS] + [(f, c) for f in ("S16LE", "F32LE", "F64LE", "S8") for c in (2, 3, 6, 8)]:
            frames = min(4096, 65536 // (VM.BPS[fmt] * ch))
            if ch > 1 and r not in (STOCK_RAMPS[1], STOCK_RAMPS[2]):
                continue
            rng = rng_for("stockg", fmt, ch, r)
            data = stock_input(fmt, rng, frames * ch)
            ones = job("F64LE", 1, frames, r, np.ones(frames, np.float64))
            cases.append((fmt, ch, frames, r, data, ones, job(fmt, ch, frames, r, data)))
    spec = tmp_path / "jobs.json"
    spec.write_text(json.dumps({"lib": os.path.join(STOCK, "lib"), "jobs": jobs}))
    r = subprocess.run([sys.executable, os.path.join(HERE, "volume_stock_child.py"), str(spec)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    switch_seen = set()
    for fmt, ch, frames, ramp_, data, ones, dst in cases:
        g = np.fromfile(ones, np.float64)
        assert g.size == frames, (fmt, ch, g.size)
        got = np.fromfile(dst, np.uint8)
        exp = VM.to_bytes(fmt, VM.gains(fmt, ch, data, g))
        assert got.size == exp.size and int((got != exp).sum()) == 0, (fmt, ch, ramp_, int((got != exp).sum()) if got.size == exp.size else got.size)
        if VM.gains(fmt, ch, data, g, doubles=False).tobytes() != VM.gains(fmt, ch, data, g, doubles=True).tobytes():
            switch_seen.add((fmt, ch))
    # the channel rule is observable on what ran: S16 and F32 on both sides of 3 channels, F64 on both sides of 2
    assert {("S16LE", 2), ("S16LE", 3), ("F32LE", 2), ("F32LE", 3), ("F64LE", 1), ("F64LE", 2)} <= switch_seen
