"""Non-interleaved (planar) layouts through the audio converter: gstamd_audio_converter_new_layouts / _samples_planes.

Nothing here needs the reference tree.  What pins the bytes is the interleaved converter, which tests/test_audio_convert.py and
tests/test_audio_convert_formats.py pin against the reference and a restatement of it:

* without a quantizer state (no dither, no noise shaping) a converter with a non-interleaved side gives the interleaved converter's output
  on the same samples, re-laid out - every container on both sides, 1 / 2 / 3 / 6 / 8 channels, frame counts that put the plane starts off
  a dword, through the mixer and the resampler too;
* with dither and / or noise shaping a non-interleaved OUTPUT is what ONE mono converter gives for plane 0 | plane 1 | ... of each call
  (gst_audio_quantize_samples walks the planes as blocks of one channel); a non-interleaved INPUT alone changes nothing;
* the passthrough and the endian shortcut hold for equal layouts only.

Inputs are finite.  Where the layouts differ the mixer runs (an identity matrix then) and decides the sign of a zero, so the inputs of float ->
float pairs whose layout changes hold no -0.0 and - since unpacking F32 to doubles turns a denormal into a signed zero - no denormals either,
except for the same-format pairs (F32 -> F32, F64 -> F64), which are mixed as they are and must keep denormals of both signs.  For the same reason -
the interleaved converter copies or byte-swaps a same-format pair, the layout-changing one unpacks and packs it - the integer inputs of a layout
change are well-formed containers: the bits above the depth of S24_32 / S20 / S18 repeat the sign (are zero for the unsigned forms), as pack writes
them; between equal layouts they are any bytes.  These are properties of the inputs: every output byte is compared.

Every check runs twice: -m "not gpu" through the kernel bodies on the host emulator (tests/emu/emu_audio_planes.cpp), -m gpu through the C ABI
on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gstreamer_amd import audio as A

BYTES = A.AFMT_BYTES
GUARD = 0xa5


class Refused(Exception):
    """(status - None on the emulator -, message)"""


def block_layout(sizes, sample_bytes, spread):
    """offsets of blocks of `sizes` bytes inside one buffer, from a 16-byte boundary: `spread` puts 5 samples of guard bytes in front of each (so that
    the blocks start off a dword for 1 / 2 / 3-byte samples), otherwise they follow each other; 32 guard bytes at both ends"""
    offs, pos = [], 32
    for s in sizes:
        if spread:
            pos += 5 * sample_bytes
        offs.append(pos)
        pos += s
    return offs, pos + 32


def fill(total, offs, blocks):
    host = np.full(total, GUARD, np.uint8)
    for o, b in zip(offs, blocks):
        host[o: o + b.size] = b
    return host


def check_guards(got, offs, sizes):
    mask = np.ones(got.size, bool)
    for o, s in zip(offs, sizes):
        mask[o: o + s] = False
    assert (got[mask] == GUARD).all(), "bytes outside the output blocks were written"


class EmuBackend:
    """tests/emu/emu_audio_planes.cpp: the rows and lanes of each launch on the host"""

    def __init__(self, emu):
        f = lambda name: getattr(emu, "emu_aconv_planes_" + name)
        f("new").restype = C.c_void_p
        f("new").argtypes = [C.c_int, C.POINTER(A.AudioInfo), C.c_int, C.POINTER(A.AudioInfo), C.c_int, C.POINTER(A.AudioConverterConfig), C.c_char_p, C.c_int]
        f("get_out_frames").restype = C.c_size_t
        f("get_out_frames").argtypes = [C.c_void_p, C.c_size_t]
        f("samples").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        f("samples_planes").argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t]
        for n in ("free", "is_passthrough", "reset"):
            f(n).argtypes = [C.c_void_p]
        self.f = f

    def new(self, ii, il, oi, ol, cfg, plain=False):
        err = C.create_string_buffer(512)
        h = self.f("new")(0, C.byref(ii), il, C.byref(oi), ol, C.byref(cfg), err, 512)
        if not h:
            raise Refused(None, err.value.decode())
        return h

    def free(self, h):
        self.f("free")(h)

    def reset(self, h):
        self.f("reset")(h)

    def out_frames(self, h, n):
        return self.f("get_out_frames")(h, n)

    def is_passthrough(self, h):
        return bool(self.f("is_passthrough")(h))

    def call(self, h, srcs, n, out_sizes, on, in_bytes, out_bytes, spread, planes):
        ioffs, itotal = block_layout([s.size for s in srcs], in_bytes, spread)
        ooffs, ototal = block_layout(out_sizes, out_bytes, spread)
        ib, ob = np.zeros(itotal + 16, np.uint8), np.zeros(ototal + 16, np.uint8)
        i0, o0 = (-ib.ctypes.data) % 16, (-ob.ctypes.data) % 16
        ib[i0: i0 + itotal] = fill(itotal, ioffs, srcs)
        ob[o0: o0 + ototal] = GUARD
        if planes:
            ip = (C.c_void_p * len(srcs))(*[ib.ctypes.data + i0 + o for o in ioffs])
            op = (C.c_void_p * len(out_sizes))(*[ob.ctypes.data + o0 + o for o in ooffs])
            self.f("samples_planes")(h, ip, n, op, on)
        else:
            self.f("samples")(h, ib.ctypes.data + i0 + ioffs[0], n, ob.ctypes.data + o0 + ooffs[0], on)
        got = ob[o0: o0 + ototal]
        check_guards(got, ooffs, out_sizes)
        return [got[o: o + s].copy() for o, s in zip(ooffs, out_sizes)]


class GpuBackend:
    """the HIP path through the C ABI"""

    def __init__(self, dev):
        self.dev = dev

    def new(self, ii, il, oi, ol, cfg, plain=False):
        from gstreamer_amd import video as V
        try:
            if plain:                           # gstamd_audio_converter_new itself
                assert il == 0 and ol == 0
                return A.AudioConverter(ii, oi, cfg)
            return A.AudioConverter(ii, oi, cfg, in_layout=il, out_layout=ol)
        except V.GstAmdError as e:
            raise Refused(e.code, str(e))

    def free(self, h):
        h.free()

    def reset(self, h):
        h.reset()

    def out_frames(self, h, n):
        return h.get_out_frames(n)

    def is_passthrough(self, h):
        return h.is_passthrough()

    def call(self, h, srcs, n, out_sizes, on, in_bytes, out_bytes, spread, planes):
        import torch
        ioffs, itotal = block_layout([s.size for s in srcs], in_bytes, spread)
        ooffs, ototal = block_layout(out_sizes, out_bytes, spread)
        ib = torch.zeros(itotal + 16, dtype=torch.uint8, device=self.dev)
        ob = torch.full((ototal + 16,), GUARD, dtype=torch.uint8, device=self.dev)
        i0, o0 = (-ib.data_ptr()) % 16, (-ob.data_ptr()) % 16
        ib[i0: i0 + itotal] = torch.from_numpy(fill(itotal, ioffs, srcs)).to(self.dev)
        if planes:
            h.samples_planes([ib.data_ptr() + i0 + o for o in ioffs], n, [ob.data_ptr() + o0 + o for o in ooffs], on)
        else:
            h.samples(ib.data_ptr() + i0 + ioffs[0], n, ob.data_ptr() + o0 + ooffs[0], on)
        torch.cuda.synchronize()
        got = ob.cpu().numpy()[o0: o0 + ototal]
        check_guards(got, ooffs, out_sizes)
        return [got[o: o + s].copy() for o, s in zip(ooffs, out_sizes)]


@pytest.fixture
def emu_backend(native_lib, emu_lib):
    return EmuBackend(emu_lib)


@pytest.fixture
def gpu_backend(native_lib, gpu):
    return GpuBackend(gpu)


# ---- layouts of a buffer ------------------------------------------------------------------------------------------------------------
def to_planes(raw, ch, b):
    """interleaved bytes -> the channels' planes"""
    m = raw.reshape(-1, ch, b)
    return [m[:, c, :].reshape(-1).copy() for c in range(ch)]


def to_frames(planes, b):
    """planes -> interleaved bytes"""
    return np.stack([p.reshape(-1, b) for p in planes], axis=1).reshape(-1).copy()


class Conv:
    """one converter; buffers go in and come out INTERLEAVED whatever its layouts, re-laid out here: .run gives the bytes an interleaved converter
    would have to give for the output to be the same samples"""

    def __init__(self, be, ifmt, ofmt, il, ol, in_ch=2, out_ch=None, in_rate=48000, out_rate=None, in_pos=None, out_pos=None, plain=False, **cfg):
        self.be, self.ifmt, self.ofmt, self.il, self.ol = be, ifmt, ofmt, il, ol
        self.in_ch, self.out_ch = in_ch, in_ch if out_ch is None else out_ch
        self.h = be.new(A.audio_info(ifmt, in_rate, in_ch, in_pos), il, A.audio_info(ofmt, out_rate or in_rate, self.out_ch, out_pos), ol,
                        A.audio_converter_config(**cfg), plain=plain)

    def run(self, raw, spread=True, planes=True):
        ib, ob = BYTES[self.ifmt], BYTES[self.ofmt]
        n = raw.size // (ib * self.in_ch)
        on = self.be.out_frames(self.h, n)
        srcs = to_planes(raw, self.in_ch, ib) if self.il else [raw]
        if not planes:
            srcs = [np.concatenate(srcs)]
        sizes = [on * ob] * self.out_ch if self.ol else [on * ob * self.out_ch]
        if not planes:
            sizes = [on * ob * self.out_ch]
        outs = self.be.call(self.h, srcs, n, sizes, on, ib, ob, spread, planes)
        if not planes and self.ol:
            outs = [outs[0][c * on * ob: (c + 1) * on * ob] for c in range(self.out_ch)]
        return to_frames(outs, ob) if self.ol else outs[0]

    def close(self):
        self.be.free(self.h)


def convert(be, ifmt, ofmt, il, ol, bufs, reset_before=(), **kw):
    c = Conv(be, ifmt, ofmt, il, ol, **kw)
    try:
        outs = []
        for k, b in enumerate(bufs):
            if k in reset_before:
                be.reset(c.h)
            outs.append(c.run(b))
        return outs, be.is_passthrough(c.h)
    finally:
        c.close()


def same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.size == e.size, (what, k, g.size, e.size)
        assert (g == e).all(), (what, k, int((g != e).sum()), g[:12], e[:12])


def reverse_samples(raw, b):
    return raw.reshape(-1, b)[:, ::-1].reshape(-1).copy()


def stream(fmt, channels, frames, seed, plain_floats=False, denormals=False):
    """interleaved frames of `fmt`: full-range random bytes for integers; finite floats in U(-1.2, 1.2) (so that clipping happens) with a sine block and
    +-1, +-0.99999999 - and, unless plain_floats, +-0.0 and single-precision denormals; `denormals`: denormals of the format itself, both signs"""
    rng = np.random.RandomState(seed)
    n = frames * channels
    if fmt[0] == "F":
        x = rng.uniform(-1.2, 1.2, n)
        x[x == 0.0] = 0.5
        x[: n // 4] = 0.9 * np.sin((np.arange(n // 4) + 1) * 0.05)
        x[x == 0.0] = 0.25
        if n >= 32:
            x[n // 2: n // 2 + 4] = [1.0, -1.0, 0.99999999, -0.99999999]
            if not plain_floats:
                x[n // 2 + 4: n // 2 + 8] = [0.0, -0.0, 1e-40, -1e-40]
        x = x.astype(np.float32 if fmt[:3] == "F32" else np.float64)
        if denormals and n >= 32:
            tiny = np.finfo(x.dtype).tiny
            x[n // 2 + 8: n // 2 + 12] = np.array([tiny / 4, -tiny / 4, tiny / 1024, -tiny / 3], x.dtype)
        raw = x.view(np.uint8).copy()
        return reverse_samples(raw, BYTES[fmt]) if fmt.endswith("BE") else raw
    return rng.randint(0, 256, n * BYTES[fmt]).astype(np.uint8)


def well_formed(raw, fmt):
    """the bits of a container above the format's depth (S24_32, S20, S18 and their unsigned forms) as pack writes them: the sign repeated, zero for
    the unsigned formats"""
    b, d = BYTES[fmt], A.AFMT_DEPTH[fmt]
    if d == 8 * b:
        return raw
    m = raw.reshape(-1, b).astype(np.uint64)
    if fmt.endswith("BE"):
        m = m[:, ::-1]
    w = sum(m[:, k] << np.uint64(8 * k) for k in range(b)) & np.uint64((1 << d) - 1)
    if fmt[0] == "S":
        w = w | (((w >> np.uint64(d - 1)) & np.uint64(1)) * np.uint64(((1 << (8 * b)) - 1) ^ ((1 << d) - 1)))
    m = np.stack([(w >> np.uint64(8 * k)) & np.uint64(0xff) for k in range(b)], axis=1).astype(np.uint8)
    if fmt.endswith("BE"):
        m = m[:, ::-1]
    return m.reshape(-1).copy()


def layout_stream(ifmt, ofmt, il, ol, ch, frames, seed):
    """the inputs of a conversion as the module's docstring sets them"""
    changes = il != ol and ifmt[0] == "F" and ofmt[0] == "F"
    raw = stream(ifmt, ch, frames, seed, plain_floats=changes, denormals=changes and ifmt == ofmt)
    # the same format, or its other byte order: the interleaved sibling copies or swaps containers that a layout change unpacks and packs, so
    # only there the bits above the depth have to be what pack writes; every other pair unpacks on both sides and keeps its random bits
    base = [f[:-2] if f[-2:] in ("LE", "BE") else f for f in (ifmt, ofmt)]
    return well_formed(raw, ifmt) if il != ol and ifmt[0] != "F" and base[0] == base[1] else raw


LAYOUTS = ((1, 1), (1, 0), (0, 1))            # every combination but interleaved -> interleaved
# every container (AKind) - 1 byte, 2 / 3 / 4 / 8 bytes in both byte orders -, unsigned and 18 / 20-bit formats among them
CONTAINERS = ("S8", "U8", "S16LE", "U16BE", "S24LE", "S20LE", "U18BE", "S32LE", "U24_32BE", "F32LE", "F32BE", "F64LE", "F64BE")
CHANNELS = (1, 2, 3, 6, 8)
FRAMES = (1, 3, 257, 1023)


# ---- 1. a permutation of the interleaved converter's output, without quantizer state -------------------------------------------------
def check_permutation(be, ifmt, ofmt, ch, frames):
    for il, ol in LAYOUTS:
        src = [layout_stream(ifmt, ofmt, il, ol, ch, frames, 31 * frames + ch + A.AFMT[ifmt])]
        exp, _ = convert(be, ifmt, ofmt, 0, 0, src, in_ch=ch, plain=True, dither_method="none")
        got, _ = convert(be, ifmt, ofmt, il, ol, src, in_ch=ch, dither_method="none")
        same(got, exp, (ifmt, ofmt, il, ol, ch, frames))


def check_container_pairs(be, ifmt):
    """every container on the other side; channel and frame counts rotate so that each format meets all of them"""
    for k, ofmt in enumerate(CONTAINERS):
        k += CONTAINERS.index(ifmt)
        check_permutation(be, ifmt, ofmt, CHANNELS[k % 5], FRAMES[(k // 5 + k) % 4])


SWEEP = (("S24LE", "F32LE"), ("F32LE", "S24BE"), ("S16LE", "S16LE"), ("F32LE", "F32LE"), ("U8", "S16LE"), ("S20LE", "U18BE"), ("F64BE", "S16LE"),
         ("S16LE", "F64LE"))


def check_sweep(be, ifmt, ofmt):
    """every channel count with every frame count (3-byte samples and odd frame counts: every plane at another offset inside a dword)"""
    for ch, frames in itertools.product(CHANNELS, FRAMES):
        check_permutation(be, ifmt, ofmt, ch, frames)


@pytest.mark.parametrize("ifmt", CONTAINERS)
def test_layouts_permute_the_interleaved_output_on_host(emu_backend, ifmt):
    check_container_pairs(emu_backend, ifmt)


@pytest.mark.gpu
@pytest.mark.parametrize("ifmt", CONTAINERS)
def test_layouts_permute_the_interleaved_output_on_device(gpu_backend, ifmt):
    check_container_pairs(gpu_backend, ifmt)


@pytest.mark.parametrize("ifmt,ofmt", SWEEP)
def test_channel_and_frame_counts_on_host(emu_backend, ifmt, ofmt):
    check_sweep(emu_backend, ifmt, ofmt)


@pytest.mark.gpu
@pytest.mark.parametrize("ifmt,ofmt", SWEEP)
def test_channel_and_frame_counts_on_device(gpu_backend, ifmt, ofmt):
    check_sweep(gpu_backend, ifmt, ofmt)


# ---- 2. the mixer and the resampler between non-interleaved sides --------------------------------------------------------------------
SURROUND = ["front-left", "front-right", "front-center", "lfe1", "rear-left", "rear-right"]


def check_mix_and_resample(be):
    sizes = (480, 333, 1, 512, 64)
    for ifmt, ofmt in (("F32LE", "S16LE"), ("S24LE", "F32LE"), ("S16LE", "S16LE"), ("F32LE", "F32LE"), ("S32LE", "S24BE")):
        for kw in (dict(in_ch=6, out_ch=2, in_pos=SURROUND), dict(in_ch=2, out_ch=6, out_pos=SURROUND), dict(in_ch=2, in_rate=48000, out_rate=44100),
                   dict(in_ch=6, out_ch=2, in_pos=SURROUND, in_rate=48000, out_rate=44100)):
            src = [stream(ifmt, kw["in_ch"], n, 5 * n + k) for k, n in enumerate(sizes)]
            exp, _ = convert(be, ifmt, ofmt, 0, 0, src, plain=True, reset_before=(3,), dither_method="none", **kw)
            assert sum(e.size for e in exp) > 0
            for il, ol in LAYOUTS:
                got, pt = convert(be, ifmt, ofmt, il, ol, src, reset_before=(3,), dither_method="none", **kw)
                assert not pt
                same(got, exp, (ifmt, ofmt, il, ol, kw))
    # the other entries work unchanged
    a = Conv(be, "F32LE", "S16LE", 0, 0, in_ch=2, in_rate=48000, out_rate=44100, plain=True)
    b = Conv(be, "F32LE", "S16LE", 1, 1, in_ch=2, in_rate=48000, out_rate=44100)
    assert [be.out_frames(a.h, n) for n in (480, 1, 37, 48000)] == [be.out_frames(b.h, n) for n in (480, 1, 37, 48000)]
    a.close()
    b.close()


def test_mix_and_resample_between_planes_on_host(emu_backend):
    check_mix_and_resample(emu_backend)


@pytest.mark.gpu
def test_mix_and_resample_between_planes_on_device(gpu_backend):
    check_mix_and_resample(gpu_backend)


@pytest.mark.gpu
def test_the_other_entries_on_a_converter_with_planes(gpu_backend):
    """get_in_frames, get_max_latency and get_mix_matrix (the C ABI has them, the host emulator does not) answer as on the interleaved converter"""
    kw = dict(in_ch=6, out_ch=2, in_pos=SURROUND, in_rate=48000, out_rate=44100)
    a = Conv(gpu_backend, "F32LE", "S16LE", 0, 0, plain=True, **kw)
    for il, ol in LAYOUTS:
        b = Conv(gpu_backend, "F32LE", "S16LE", il, ol, **kw)
        assert [b.h.get_in_frames(n) for n in (441, 1, 37, 44100)] == [a.h.get_in_frames(n) for n in (441, 1, 37, 44100)]
        assert b.h.get_max_latency() == a.h.get_max_latency() > 0
        m = b.h.mix_matrix(6, 2)
        assert m == a.h.mix_matrix(6, 2) and any(v != 0.0 for row in m for v in row)
        b.close()
    a.close()


# ---- 3. the quantizer of a non-interleaved output is a mono quantizer over plane 0 | plane 1 | ... -------------------------------------
QUANT = [(d, "none") for d in ("rpdf", "tpdf", "tpdf-hf")] + [(d, ns) for d in ("none", "tpdf") for ns in ("error-feedback", "simple", "medium", "high")]
CALLS = (333, 64, 1)


def check_mono_relation(be, dither, ns):
    cfg = dict(dither_method=dither, noise_shaping=ns)
    for ifmt, ofmt, ch in itertools.product(("F32LE", "S32LE"), ("S16LE", "S8", "S20LE"), (2, 6)):
        src = [stream(ifmt, ch, n, 3 * n + ch + A.AFMT[ofmt]) for n in CALLS]
        ib, ob = BYTES[ifmt], BYTES[ofmt]
        mono_in = [np.concatenate(to_planes(b, ch, ib)) for b in src]
        mono, _ = convert(be, ifmt, ofmt, 0, 0, mono_in, in_ch=1, plain=True, **cfg)
        exp = [to_frames(np.split(m, ch), ob) for m in mono]
        for il in (0, 1):
            got, _ = convert(be, ifmt, ofmt, il, 1, src, in_ch=ch, **cfg)
            same(got, exp, ("mono relation", ifmt, ofmt, ch, il, dither, ns))
        # the interleaved quantizer is another one (so the relation above is not trivially true) ...
        inter, _ = convert(be, ifmt, ofmt, 0, 0, src, in_ch=ch, plain=True, **cfg)
        assert any((a != b).any() for a, b in zip(inter, exp)), (ifmt, ofmt, ch, dither, ns)
        # ... and a non-interleaved INPUT does not touch it
        got, _ = convert(be, ifmt, ofmt, 1, 0, src, in_ch=ch, **cfg)
        same(got, inter, ("planar input, interleaved quantizer", ifmt, ofmt, ch, dither, ns))


@pytest.mark.parametrize("dither,ns", QUANT)
def test_planar_output_is_quantized_as_one_channel_on_host(emu_backend, dither, ns):
    check_mono_relation(emu_backend, dither, ns)


@pytest.mark.gpu
@pytest.mark.parametrize("dither,ns", QUANT)
def test_planar_output_is_quantized_as_one_channel_on_device(gpu_backend, dither, ns):
    check_mono_relation(gpu_backend, dither, ns)


# ---- 4. the passthrough and the endian plan ----------------------------------------------------------------------------------------
def f32_specials(frames, ch):
    w = np.array([0x00000001, 0x007fffff, 0x80000001, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc12345, 0xffc54321, 0x7f812345,
                  0xff8abcde, 0x3f800000, 0xbf800000, 0x00800000, 0x12345678], np.uint32)
    return np.tile(w, frames * ch // 16 + 1)[: frames * ch].view(np.uint8).copy()


def check_shortcuts(be):
    for fmt, ch, frames in (("S24BE", 3, 67), ("F32LE", 2, 67), ("U8", 6, 5), ("F64BE", 8, 1), ("S16LE", 2, 333)):
        raw = f32_specials(frames, ch) if fmt == "F32LE" else stream(fmt, ch, frames, frames)
        got, pt = convert(be, fmt, fmt, 1, 1, [raw], in_ch=ch, dither_method="tpdf", noise_shaping="high")
        assert pt, (fmt, "the same format, channels and layout is a passthrough")
        same(got, [raw], (fmt, "plane by plane through plane pointers that are not contiguous"))
        for il, ol in ((1, 0), (0, 1)):
            _, pt = convert(be, fmt, fmt, il, ol, [stream(fmt, ch, frames, 1, plain_floats=True)], in_ch=ch)
            assert not pt, (fmt, il, ol, "a layout change is not a passthrough")
    # the endian shortcut between two non-interleaved sides keeps NaN payloads and denormals, as between two interleaved ones
    le = f32_specials(67, 2)
    for planes in (True, False):                # plane by plane; one launch over contiguous planes
        for x, y in (("F32LE", "F32BE"), ("F32BE", "F32LE")):
            c = Conv(be, x, y, 1, 1)
            got, pt = c.run(le, spread=planes, planes=planes), be.is_passthrough(c.h)
            c.close()
            assert not pt
            same([got], [reverse_samples(le, 4)], (x, y, planes, "a byte swap"))
    # the generic chain flushes the denormals of the same buffer: the two paths can be told apart
    f64, _ = convert(be, "F32LE", "F64LE", 1, 1, [le])
    x = le.view(np.uint32)
    den = ((x & 0x7f800000) == 0) & ((x & 0x007fffff) != 0)
    assert den.any() and (f64[0].view(np.float64)[den] == 0.0).all()
    for a, ch, n in (("S16", 2, 333), ("U24", 3, 67), ("S20", 6, 5), ("U24_32", 2, 64), ("S32", 8, 3)):
        raw = stream(a + "LE", ch, n, n)
        got, pt = convert(be, a + "LE", a + "BE", 1, 1, [raw], in_ch=ch, dither_method="tpdf", noise_shaping="high")
        assert not pt
        same(got, [reverse_samples(raw, BYTES[a + "LE"])], (a, ch, n))
    # with a layout change the same pair is the generic chain: its output is the interleaved generic chain's - which for an integer pair is the
    # swap again, bit for bit (24 bits unpacked, mixed by 1024 and packed are the same 24 bits)
    raw = stream("S24LE", 2, 67, 9)
    for il, ol in ((1, 0), (0, 1)):
        got, pt = convert(be, "S24LE", "S24BE", il, ol, [raw], dither_method="tpdf")
        assert not pt
        same(got, [reverse_samples(raw, 3)], ("S24LE -> S24BE", il, ol))


def test_passthrough_and_endian_plan_on_host(emu_backend):
    check_shortcuts(emu_backend)


@pytest.mark.gpu
def test_passthrough_and_endian_plan_on_device(gpu_backend):
    check_shortcuts(gpu_backend)


# ---- 5. samples and samples_planes ----------------------------------------------------------------------------------------------------
def check_samples_vs_planes(be):
    """contiguous planes through samples, the same planes with guard bytes between them through samples_planes: identical bytes, none outside the
    planes (the backends check the guard bytes around every output block of every call in this file)"""
    for ifmt, ofmt, il, ol, ch, cfg in (("F32LE", "S16LE", 1, 1, 2, dict(dither_method="tpdf", noise_shaping="high")),
                                        ("S24LE", "F32LE", 0, 1, 3, {}), ("F32LE", "S24BE", 1, 0, 6, dict(dither_method="rpdf")),
                                        ("S16LE", "S16LE", 1, 1, 2, {}), ("U8", "S8", 1, 1, 8, {}), ("F64LE", "F64BE", 1, 1, 2, {}),
                                        ("S20LE", "S18LE", 1, 1, 3, dict(dither_method="tpdf-hf"))):
        src = [stream(ifmt, ch, n, n + ch, plain_floats=True) for n in (257, 3, 1023)]
        a, b = Conv(be, ifmt, ofmt, il, ol, in_ch=ch, **cfg), Conv(be, ifmt, ofmt, il, ol, in_ch=ch, **cfg)
        try:
            same([a.run(s, spread=False, planes=False) for s in src], [b.run(s, spread=True, planes=True) for s in src], (ifmt, ofmt, il, ol, ch))
        finally:
            a.close()
            b.close()


def test_samples_and_samples_planes_agree_on_host(emu_backend):
    check_samples_vs_planes(emu_backend)


@pytest.mark.gpu
def test_samples_and_samples_planes_agree_on_device(gpu_backend):
    check_samples_vs_planes(gpu_backend)


def check_layouts_zero_is_new(be):
    """new_layouts (.., 0, .., 0, ..) makes the converter gstamd_audio_converter_new makes"""
    for ifmt, ofmt, cfg in (("F32LE", "S16LE", dict(dither_method="tpdf", noise_shaping="high")), ("S24BE", "F32LE", {}), ("S16LE", "S16LE", {}),
                            ("F32LE", "U18BE", dict(dither_method="tpdf-hf")), ("F32LE", "F32BE", {})):
        src = [stream(ifmt, 2, n, n) for n in (333, 64, 1)]
        a, pa = convert(be, ifmt, ofmt, 0, 0, src, plain=True, **cfg)
        b, pb = convert(be, ifmt, ofmt, 0, 0, src, **cfg)
        assert pa == pb
        same(b, a, (ifmt, ofmt))


def test_interleaved_layouts_make_the_old_converter_on_host(native_lib, emu_lib):
    """on the host `plain` is the same entry: compare with the interleaved-only emulator (prefix emu_aconv_lanes_) instead"""
    from test_audio_convert_formats import EmuBackend as Lanes, run
    be = EmuBackend(emu_lib)
    for ifmt, ofmt, cfg in (("F32LE", "S16LE", dict(dither_method="tpdf", noise_shaping="high")), ("S24BE", "F32LE", {}), ("S16LE", "S16LE", {}),
                            ("F32LE", "U18BE", dict(dither_method="tpdf-hf")), ("F32LE", "F32BE", {})):
        src = [stream(ifmt, 2, n, n) for n in (333, 64, 1)]
        a, pa = run(Lanes(emu_lib), ifmt, ofmt, src, **cfg)
        b, pb = convert(be, ifmt, ofmt, 0, 0, src, **cfg)
        assert pa == pb
        same(b, a, (ifmt, ofmt))


@pytest.mark.gpu
def test_interleaved_layouts_make_the_old_converter_on_device(gpu_backend):
    check_layouts_zero_is_new(gpu_backend)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def check_refusals(be, codes):
    good = A.audio_info("S16LE", 48000, 2)
    cfg = A.audio_converter_config()
    for il, ol in ((2, 0), (0, 2), (-1, 1), (1, 7)):
        with pytest.raises(Refused) as r:
            be.new(good, il, good, ol, cfg)
        assert r.value.args[0] in codes and r.value.args[1]
    for fmt in ("S16LE", "S24BE"):
        planar = A.audio_info(fmt, 48000, 2)
        planar.layout = 1
        for ii, oi in ((planar, A.audio_info(fmt, 48000, 2)), (A.audio_info(fmt, 48000, 2), planar)):
            for il, ol in ((0, 0), (1, 1), (1, 0)):
                with pytest.raises(Refused) as r:
                    be.new(ii, il, oi, ol, cfg)
                assert r.value.args[0] in codes and r.value.args[1]


def test_refusals_on_host(emu_backend):
    check_refusals(emu_backend, (None,))


@pytest.mark.gpu
def test_refusals_on_device(gpu_backend):
    from gstreamer_amd import video as V
    check_refusals(gpu_backend, (V.ERR_UNSUPPORTED, V.ERR_INVALID))
    # what tests/test_audio_convert_formats.py pins: gstamd_audio_converter_new itself keeps refusing GstAmdAudioInfo.layout = 1
    planar = A.audio_info("S16LE", 48000, 2)
    planar.layout = 1
    for ii, oi in ((planar, A.audio_info("S16LE", 48000, 2)), (A.audio_info("S16LE", 48000, 2), planar)):
        with pytest.raises(V.GstAmdError) as r:
            A.AudioConverter(ii, oi, A.audio_converter_config())
        assert r.value.code == V.ERR_UNSUPPORTED and str(r.value)


def test_the_old_constructor_keeps_refusing_a_layout_on_host(native_lib, emu_lib):
    """aconv_make_plan, which the interleaved-only emulator entry goes through"""
    from test_audio_convert_formats import EmuBackend as Lanes, Refused as LanesRefused
    planar = A.audio_info("S16LE", 48000, 2)
    planar.layout = 1
    for ii, oi in ((planar, A.audio_info("S16LE", 48000, 2)), (A.audio_info("S16LE", 48000, 2), planar)):
        with pytest.raises(LanesRefused) as r:
            Lanes(emu_lib).new(ii, oi, A.audio_converter_config())
        assert r.value.args[1]
