"""The audio converter over every raw GstAudioFormat (values 2 .. 31): the big-endian, unsigned and 18 / 20-bit formats next to the eight it started with.

Nothing here needs the reference tree.  What pins the bytes:

* a numpy restatement, written below from the rules of audio-format.c's unpack / pack with GST_AUDIO_PACK_FLAG_TRUNCATE_RANGE (plain shifts)
  and of gst_audio_quantize_quantize_int_none_none (add half a step with saturation, clear the bits below the depth), for conversions without
  dither between every integer format and S32LE / F64LE;
* the little-endian paths that tests/test_audio_convert.py compares with the reference: a big-endian format must give the bytes of its
  little-endian sibling reversed per sample, an unsigned one the bytes of its signed sibling with the sign bit flipped - with dither and noise
  shaping, over consecutive buffers of one converter.  S20LE and S18LE have no sibling that was there before: they are pinned absolutely by
  the restatement without dither only, and their three siblings each (BE, U, UBE) are checked against them with dither;
* for the endian shortcut (formats that differ in byte order only, no mix, no rate change): an exact byte swap, NaN payloads and denormals
  included, which the generic chain (shown on the same buffer through F32LE -> F64LE) would flush.

Every check runs twice: -m "not gpu" through the kernel bodies on the host emulator, -m gpu through the C ABI on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gstreamer_amd import audio as A

BYTES = A.AFMT_BYTES
INT_FORMATS = [f for f in A.AFMT if f[0] in "SU"]
OLD_FORMATS = ["S8", "U8", "S16LE", "S24LE", "S24_32LE", "S32LE", "F32LE", "F64LE"]
NEW_FORMATS = [f for f in A.AFMT if f not in OLD_FORMATS]
NEW_INT_FORMATS = [f for f in NEW_FORMATS if f[0] in "SU"]
BE_FORMATS = [f for f in A.AFMT if f.endswith("BE")]
UNSIGNED_LE = [f for f in NEW_FORMATS if f[0] == "U" and f.endswith("LE")]


def test_the_format_tables_hold_every_raw_format():
    """GstAudioFormat 2 .. 31 (0 is UNKNOWN, 1 ENCODED): 30 raw formats, 22 of them new here"""
    assert sorted(A.AFMT.values()) == list(range(2, 32))
    assert len(NEW_FORMATS) == 22 and len(NEW_INT_FORMATS) == 20 and len(BE_FORMATS) == 14
    assert A.AFMT["S16BE"] == 5 and A.AFMT["U24_32BE"] == 11 and A.AFMT["S24BE"] == 17 and A.AFMT["U18BE"] == 27 and A.AFMT["F64BE"] == 31
    assert BYTES["S20LE"] == 3 and BYTES["U24_32LE"] == 4 and BYTES["U16BE"] == 2 and BYTES["F64BE"] == 8


# ---- the formats restated ---------------------------------------------------------------------------------------------------------
def depth(fmt):
    return A.AFMT_DEPTH[fmt]


def containers(raw, fmt):
    """the samples' containers as unsigned integers, read in the format's byte order"""
    b = BYTES[fmt]
    m = raw.reshape(-1, b).astype(np.uint64)
    if fmt.endswith("BE"):
        m = m[:, ::-1]
    return sum(m[:, k] << np.uint64(8 * k) for k in range(b)) if b else m


def container_bytes(w, fmt):
    b = BYTES[fmt]
    m = np.stack([(w >> np.uint64(8 * k)) & np.uint64(0xff) for k in range(b)], axis=1).astype(np.uint8)
    if fmt.endswith("BE"):
        m = m[:, ::-1]
    return m.reshape(-1).copy()


def unpack_s32(raw, fmt):
    """(int32) (w << (32 - depth)), sign bit flipped for the unsigned formats; container bits above the depth fall off the top"""
    w = (containers(raw, fmt) << np.uint64(32 - depth(fmt))) & np.uint64(0xffffffff)
    if fmt[0] == "U":
        w = w ^ np.uint64(0x80000000)
    return w.astype(np.uint32).view(np.int32)


def quantize_none(v, d):
    """gst_audio_quantize_quantize_int_none_none: half a quantiser step added with saturation, the bits below the depth cleared"""
    if d >= 32:
        return v
    shift = 32 - d
    s = np.minimum(v.astype(np.int64) + (1 << (shift - 1)), 2147483647)
    return (s & ~((1 << shift) - 1)).astype(np.int32)


def pack_s32(v, fmt):
    """signed: v >> (32 - depth) arithmetic, the container's low bytes; unsigned: sign bit flipped, logical shift"""
    shift = 32 - depth(fmt)
    if fmt[0] == "U":
        w = (v.view(np.uint32).astype(np.uint64) ^ np.uint64(0x80000000)) >> np.uint64(shift)
    else:
        w = (v.astype(np.int64) >> shift).astype(np.uint64) & np.uint64((1 << (8 * BYTES[fmt])) - 1)
    return container_bytes(w, fmt)


def reverse_samples(raw, b):
    return raw.reshape(-1, b)[:, ::-1].reshape(-1).copy()


def flip_sign(raw, fmt):
    """a container of the signed sibling <-> of the unsigned format `fmt`: the top used bit flipped, the spare bits above it zero"""
    d = depth(fmt)
    w = (containers(raw, fmt) & np.uint64((1 << d) - 1)) ^ np.uint64(1 << (d - 1))
    return container_bytes(w, fmt)


def sign_extended(raw, fmt):
    """the spare bits of a signed container (S24_32, S20, S18) repeat the sign"""
    d, bits = depth(fmt), 8 * BYTES[fmt]
    w = containers(raw, fmt)
    spare = w >> np.uint64(d)
    sign = (w >> np.uint64(d - 1)) & np.uint64(1)
    return bool((spare == sign * np.uint64((1 << (bits - d)) - 1)).all())


def stream(fmt, channels, frames, seed):
    """interleaved frames of `fmt`: full-range random bytes for integers, U(-1.2, 1.2) (so that clipping happens) and a sine block for floats"""
    rng = np.random.RandomState(seed)
    n = frames * channels
    if fmt[0] == "F":
        x = rng.uniform(-1.2, 1.2, n)
        x[: n // 4] = 0.9 * np.sin(np.arange(n // 4) * 0.05)
        if n >= 32:
            x[n // 2: n // 2 + 8] = [0.0, -0.0, 1.0, -1.0, 1e-40, -1e-40, 0.99999999, -0.99999999]
        raw = x.astype(np.float32 if fmt[:3] == "F32" else np.float64).view(np.uint8).copy()
        return reverse_samples(raw, BYTES[fmt]) if fmt.endswith("BE") else raw
    return rng.randint(0, 256, n * BYTES[fmt]).astype(np.uint8)


# ---- the two ways to run a converter ----------------------------------------------------------------------------------------------
class Refused(Exception):
    """(status of gstamd_audio_converter_new - None on the emulator, which has the plan's verdict only -, message)"""


class EmuBackend:
    """the kernel bodies on the host: tests/emu/emu_audio_lanes.cpp walks the lanes of each launch (prefix "emu_aconv_lanes_"), tests/emu/emu_audio.cpp
    walks samples (prefix "emu_aconv_")"""

    def __init__(self, emu, prefix="emu_aconv_lanes_"):
        f = lambda name: getattr(emu, prefix + name)
        f("new").restype = C.c_void_p
        f("new").argtypes = [C.c_int, C.POINTER(A.AudioInfo), C.POINTER(A.AudioInfo), C.POINTER(A.AudioConverterConfig), C.c_char_p, C.c_int]
        f("get_out_frames").restype = C.c_size_t
        f("get_out_frames").argtypes = [C.c_void_p, C.c_size_t]
        f("samples").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        f("free").argtypes = [C.c_void_p]
        f("is_passthrough").argtypes = [C.c_void_p]
        self.f = f

    def new(self, ii, oi, cfg):
        err = C.create_string_buffer(512)
        h = self.f("new")(0, C.byref(ii), C.byref(oi), C.byref(cfg), err, 512)
        if not h:
            raise Refused(None, err.value.decode())
        return h

    def free(self, h):
        self.f("free")(h)

    def out_frames(self, h, n):
        return self.f("get_out_frames")(h, n)

    def is_passthrough(self, h):
        return bool(self.f("is_passthrough")(h))

    def samples(self, h, src, n, out_bytes, in_off=0, out_off=0):
        """in_off / out_off: the buffers start that many bytes past a 16-byte boundary"""
        on = self.out_frames(h, n)
        ib, ob = np.zeros(src.size + 32, np.uint8), np.full(on * out_bytes + 32, 0xa5, np.uint8)
        i0 = (-ib.ctypes.data) % 16 + in_off
        o0 = (-ob.ctypes.data) % 16 + out_off
        ib[i0: i0 + src.size] = src
        self.f("samples")(h, ib.ctypes.data + i0, n, ob.ctypes.data + o0, on)
        assert (ob[:o0] == 0xa5).all() and (ob[o0 + on * out_bytes:] == 0xa5).all(), "bytes outside the output were written"
        return ob[o0: o0 + on * out_bytes].copy()


class GpuBackend:
    """the HIP path through the C ABI"""

    def __init__(self, dev):
        self.dev = dev

    def new(self, ii, oi, cfg):
        from gstreamer_amd import video as V
        try:
            return A.AudioConverter(ii, oi, cfg)
        except V.GstAmdError as e:
            raise Refused(e.code, str(e))

    def free(self, h):
        h.free()

    def out_frames(self, h, n):
        return h.get_out_frames(n)

    def is_passthrough(self, h):
        return h.is_passthrough()

    def samples(self, h, src, n, out_bytes, in_off=0, out_off=0):
        import torch
        on = self.out_frames(h, n)
        ib = torch.zeros(src.size + 32, dtype=torch.uint8, device=self.dev)
        ob = torch.full((on * out_bytes + 32,), 0xa5, dtype=torch.uint8, device=self.dev)
        i0 = (-ib.data_ptr()) % 16 + in_off
        o0 = (-ob.data_ptr()) % 16 + out_off
        if src.size:
            ib[i0: i0 + src.size] = torch.from_numpy(src).to(self.dev)
        h.samples(ib[i0:], n, ob[o0:], on)
        torch.cuda.synchronize()
        got = ob.cpu().numpy()
        assert (got[:o0] == 0xa5).all() and (got[o0 + on * out_bytes:] == 0xa5).all(), "bytes outside the output were written"
        return got[o0: o0 + on * out_bytes].copy()


@pytest.fixture
def emu_backend(native_lib, emu_lib):
    return EmuBackend(emu_lib)


@pytest.fixture
def gpu_backend(native_lib, gpu):
    return GpuBackend(gpu)


def run(be, ifmt, ofmt, bufs, in_ch=2, out_ch=None, in_rate=48000, out_rate=None, in_off=0, out_off=0, **cfg):
    """the buffers of `bufs` (uint8 arrays) through one converter; returns the outputs and the converter's is_passthrough"""
    out_ch = in_ch if out_ch is None else out_ch
    h = be.new(A.audio_info(ifmt, in_rate, in_ch), A.audio_info(ofmt, out_rate or in_rate, out_ch), A.audio_converter_config(**cfg))
    try:
        outs = [be.samples(h, b, b.size // (BYTES[ifmt] * in_ch), BYTES[ofmt] * out_ch, in_off, out_off) for b in bufs]
        return outs, be.is_passthrough(h)
    finally:
        be.free(h)


def same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.size == e.size, (what, k, g.size, e.size)
        assert (g == e).all(), (what, k, int((g != e).sum()), g[:12], e[:12])


SIZES = (1024, 333, 1, 0)


# ---- 1. against the restatement: no dither, to and from S32LE and F64LE -----------------------------------------------------------
def check_restated(be, fmt):
    for ch in (1, 2):
        src = [stream(fmt, ch, n, 7 * n + ch + A.AFMT[fmt]) for n in SIZES]
        s32 = [unpack_s32(b, fmt) for b in src]
        got, _ = run(be, fmt, "S32LE", src, in_ch=ch, dither_method="none")
        same(got, [v.view(np.uint8) for v in s32], (fmt, "-> S32LE", ch))
        # X -> F64LE is the S32LE -> F64LE conversion of the restated samples
        got, _ = run(be, fmt, "F64LE", src, in_ch=ch, dither_method="none")
        exp, _ = run(be, "S32LE", "F64LE", [v.view(np.uint8).copy() for v in s32], in_ch=ch, dither_method="none")
        same(got, exp, (fmt, "-> F64LE", ch))
        for v, e in zip(s32, exp):              # and that one is v / 2^31, exact in double
            assert (e.view(np.float64) == v.astype(np.float64) / 2147483648.0).all()
        src32 = [stream("S32LE", ch, n, 11 * n + ch + A.AFMT[fmt]) for n in SIZES]
        got, _ = run(be, "S32LE", fmt, src32, in_ch=ch, dither_method="none")
        same(got, [pack_s32(quantize_none(b.view(np.int32), depth(fmt)), fmt) for b in src32], ("S32LE ->", fmt, ch))
        # F64LE -> X is the restated quantise and pack of the F64LE -> S32LE conversion
        src64 = [stream("F64LE", ch, n, 13 * n + ch + A.AFMT[fmt]) for n in SIZES]
        mid, _ = run(be, "F64LE", "S32LE", src64, in_ch=ch, dither_method="none")
        got, _ = run(be, "F64LE", fmt, src64, in_ch=ch, dither_method="none")
        same(got, [pack_s32(quantize_none(b.view(np.int32), depth(fmt)), fmt) for b in mid], ("F64LE ->", fmt, ch))


@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_integer_formats_match_the_restatement_on_host(emu_backend, fmt):
    check_restated(emu_backend, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_integer_formats_match_the_restatement_on_device(gpu_backend, fmt):
    check_restated(gpu_backend, fmt)


# ---- 2. against the little-endian / signed siblings, with dither and noise shaping -------------------------------------------------
DITHERS = ("none", "tpdf", "tpdf-hf")
SHAPINGS = ("none", "high")
SPREAD = ("F32LE", "S32LE", "S16LE")
BUFS3 = (512, 333, 64)


def sibling_of(fmt):
    """(sibling, its bytes -> this format's bytes): BE formats go back to their LE form, unsigned LE ones to the signed LE form"""
    if fmt.endswith("BE"):
        return fmt[:-2] + "LE", lambda raw: reverse_samples(raw, BYTES[fmt])
    return "S" + fmt[1:], lambda raw: flip_sign(raw, fmt)


def check_sibling(be, fmt, dither, ns):
    """One pair has no sibling conversion to compare with as it stands: S16LE <-> U16LE against S16LE -> S16LE, which is the passthrough copy
    while the unsigned side runs the chain (S32 in between, so the 16-bit output is dithered - the reference's own plan).  There the sibling
    conversion is the pinned S32LE -> S16LE of the same samples widened to S32 (v << 16), which is what the chain sees."""
    sib, to_fmt = sibling_of(fmt)
    cfg = dict(dither_method=dither, noise_shaping=ns)
    for other in SPREAD:
        chain_src = other
        widen = lambda b: b
        if other == sib and not fmt.endswith("BE"):
            chain_src, widen = "S32LE", lambda b: unpack_s32(b, sib).view(np.uint8).copy()
        src = [stream(other, 2, n, 3 * n + A.AFMT[fmt]) for n in BUFS3]
        got, _ = run(be, other, fmt, src, **cfg)
        exp, _ = run(be, chain_src, sib, [widen(b) for b in src], **cfg)
        if sib[0] == "S" and sib[0] != fmt[0]:
            assert all(sign_extended(e, sib) for e in exp), (other, sib, "spare bits")
        same(got, [to_fmt(e) for e in exp], (other, "->", fmt, "vs", sib, dither, ns))
        raw = [stream(sib, 2, n, 5 * n + A.AFMT[fmt]) for n in BUFS3]
        got, _ = run(be, fmt, other, [to_fmt(b) for b in raw], **cfg)
        exp, _ = run(be, chain_src if chain_src != other else sib, other, [widen(b) for b in raw], **cfg)
        same(got, exp, (fmt, "->", other, "vs", sib, dither, ns))


SIBLING_CASES = list(itertools.product(BE_FORMATS + UNSIGNED_LE, DITHERS, SHAPINGS))


@pytest.mark.parametrize("fmt,dither,ns", SIBLING_CASES)
def test_formats_match_their_pinned_siblings_on_host(emu_backend, fmt, dither, ns):
    check_sibling(emu_backend, fmt, dither, ns)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,dither,ns", SIBLING_CASES)
def test_formats_match_their_pinned_siblings_on_device(gpu_backend, fmt, dither, ns):
    check_sibling(gpu_backend, fmt, dither, ns)


def check_dither_threshold(be):
    """chain_quantize drops the dither where the output depth is ABOVE dither-threshold (audio-converter.c: out_depth > threshold; the element's
    property text says "at/below which to apply dithering"): at the default of 20 both S18 and S20 are dithered and S24 is not, at 19 S20 is not
    either - straight from the format table's depth, with no decision code of its own."""
    src = [stream("F32LE", 2, 512, 99)]
    for fmt, threshold, differs in (("S18LE", 20, True), ("S20LE", 20, True), ("U18BE", 20, True), ("U20BE", 20, True), ("U24BE", 20, False),
                                    ("S20LE", 19, False), ("U20BE", 19, False), ("S18BE", 19, True), ("S18BE", 17, False)):
        a, _ = run(be, "F32LE", fmt, src, dither_method="none", dither_threshold=threshold)
        b, _ = run(be, "F32LE", fmt, src, dither_method="tpdf", dither_threshold=threshold)
        assert bool((a[0] != b[0]).any()) == differs, (fmt, threshold)


def test_dither_threshold_follows_the_depth_on_host(emu_backend):
    check_dither_threshold(emu_backend)


@pytest.mark.gpu
def test_dither_threshold_follows_the_depth_on_device(gpu_backend):
    check_dither_threshold(gpu_backend)


# ---- 3. the endian shortcut ---------------------------------------------------------------------------------------------------------
def f32_specials():
    w = np.array([0x00000001, 0x007fffff, 0x80000001, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc12345, 0xffc54321, 0x7f812345,
                  0xff8abcde, 0x3f800000, 0xbf800000, 0x00800000, 0x12345678], np.uint32)
    return np.tile(w, 9)[: 2 * 67].view(np.uint8).copy()          # 67 stereo frames: a head / tail for the four-sample lanes too


def check_endian_shortcut(be):
    le = f32_specials()
    got, pt = run(be, "F32LE", "F32BE", [le])
    assert not pt
    same(got, [reverse_samples(le, 4)], "F32LE -> F32BE is a byte swap")
    back, pt = run(be, "F32BE", "F32LE", got)
    assert not pt
    same(back, [le], "F32BE -> F32LE is a byte swap")
    # the generic chain flushes the denormals of the same buffer: the two paths can be told apart
    f64, _ = run(be, "F32LE", "F64LE", [le])
    x = le.view(np.uint32)
    den = ((x & 0x7f800000) == 0) & ((x & 0x007fffff) != 0)
    assert den.any() and (f64[0].view(np.float64)[den] == 0.0).all()
    # doubles with payloads, integers of every container
    d = np.array([0x0000000000000001, 0x800fffffffffffff, 0x7ff8000000012345, 0xfff4000000054321, 0x7ff0000000000000, 0x3ff0000000000000], np.uint64)
    d = np.tile(d, 23)[: 2 * 67].view(np.uint8).copy()
    same(run(be, "F64LE", "F64BE", [d])[0], [reverse_samples(d, 8)], "F64LE -> F64BE")
    same(run(be, "F64BE", "F64LE", [d])[0], [reverse_samples(d, 8)], "F64BE -> F64LE")
    for a in ("S16", "U16", "S24", "U24", "S20", "U20", "S18", "U18", "S24_32", "U24_32", "S32", "U32"):
        for x, y in ((a + "LE", a + "BE"), (a + "BE", a + "LE")):
            for n in (1024, 333, 1, 0):
                raw = stream(x, 2, n, n + A.AFMT[x])
                got, pt = run(be, x, y, [raw], dither_method="tpdf", noise_shaping="high")     # neither applies: nothing is quantised
                assert not pt
                same(got, [reverse_samples(raw, BYTES[x])], (x, "->", y, n))
    # with a mix or a rate change the same pair goes through the generic chain: the LE-path relation.  S16LE -> S16LE and F32LE -> F32LE are
    # not that chain (the same intermediate format on both sides is mixed and resampled as it is, in 16 bits / single precision), so for
    # these the LE path is S32LE -> S16LE / F64LE -> F32LE of the samples widened the way unpack does
    def widened(x, raw):
        if x == "S16LE":
            return "S32LE", unpack_s32(raw, x).view(np.uint8).copy()
        if x == "F32LE":
            f = raw.view(np.float32).astype(np.float64)
            den = (raw.view(np.uint32) & 0x7f800000) == 0
            f[den] = np.copysign(0.0, f[den])           # audio_orc_unpack_f32 flushes denormals
            return "F64LE", f.view(np.uint8).copy()
        return x, raw

    for kw in (dict(in_ch=2, out_ch=1), dict(in_rate=48000, out_rate=44100)):
        for x, y in (("S16LE", "S16BE"), ("S16BE", "S16LE"), ("S24BE", "S24LE"), ("F32LE", "F32BE"), ("F32BE", "F32LE"), ("U20LE", "U20BE")):
            raw = [stream(x, 2, 480, 21 + k) for k in range(3)]
            got, pt = run(be, x, y, raw, **kw)
            assert not pt
            xl, yl = x[:-2] + "LE", y[:-2] + "LE"
            le_in = [widened(xl, reverse_samples(b, BYTES[x]) if x.endswith("BE") else b) for b in raw]
            exp, _ = run(be, le_in[0][0], yl, [b for _, b in le_in], **kw)
            same(got, [reverse_samples(e, BYTES[y]) if y.endswith("BE") else e for e in exp], (x, "->", y, kw))


def test_endian_pairs_are_byte_swaps_on_host(emu_backend):
    check_endian_shortcut(emu_backend)


@pytest.mark.gpu
def test_endian_pairs_are_byte_swaps_on_device(gpu_backend):
    check_endian_shortcut(gpu_backend)


# ---- 4. mix and resample through a new format ---------------------------------------------------------------------------------------
def check_resample_down_mix(be):
    """tests/test_audio_convert.py's s24_s16_resample_down_mix in big-endian: the LE case's output reversed, buffer by buffer"""
    raw = [stream("S24LE", 2, 960, 1000 + 17 * k) for k in range(4)]
    kw = dict(in_ch=2, out_ch=1, in_rate=48000, out_rate=16000)
    exp, _ = run(be, "S24LE", "S16LE", raw, **kw)
    got, _ = run(be, "S24BE", "S16BE", [reverse_samples(b, 3) for b in raw], **kw)
    assert sum(e.size for e in exp) > 0
    same(got, [reverse_samples(e, 2) for e in exp], "S24BE 48k stereo -> S16BE 16k mono")
    hl = be.new(A.audio_info("S24LE", 48000, 2), A.audio_info("S16LE", 16000, 1), A.audio_converter_config())
    hb = be.new(A.audio_info("S24BE", 48000, 2), A.audio_info("S16BE", 16000, 1), A.audio_converter_config())
    assert [be.out_frames(hl, n) for n in (960, 1, 37, 48000)] == [be.out_frames(hb, n) for n in (960, 1, 37, 48000)]
    be.free(hl)
    be.free(hb)


def test_mix_and_resample_through_big_endian_on_host(emu_backend):
    check_resample_down_mix(emu_backend)


@pytest.mark.gpu
def test_mix_and_resample_through_big_endian_on_device(gpu_backend):
    check_resample_down_mix(gpu_backend)


# ---- 5. refusals stay refusals ------------------------------------------------------------------------------------------------------
def check_refusals(be):
    from gstreamer_amd import video as V
    good = A.audio_info("S16LE", 48000, 2)
    for value in (0, 1, 32, 33, 100, -1):                # UNKNOWN, ENCODED, past the last raw format
        bad = A.audio_info("S16LE", 48000, 2)
        bad.format = value
        for ii, oi in ((bad, good), (good, bad)):
            with pytest.raises(Refused) as r:
                be.new(ii, oi, A.audio_converter_config())
            assert r.value.args[0] in (None, V.ERR_UNSUPPORTED) and r.value.args[1]
    for fmt in ("S16LE", "S24BE"):
        planar = A.audio_info(fmt, 48000, 2)
        planar.layout = 1
        for ii, oi in ((planar, A.audio_info(fmt, 48000, 2)), (A.audio_info(fmt, 48000, 2), planar)):
            with pytest.raises(Refused) as r:
                be.new(ii, oi, A.audio_converter_config())
            assert r.value.args[0] in (None, V.ERR_UNSUPPORTED) and r.value.args[1]
    for x, y, expect in (("S24BE", "S24BE", True), ("U20LE", "U20LE", True), ("F64BE", "F64BE", True), ("S24BE", "S24LE", False), ("S16LE", "U16LE", False),
                         ("F32BE", "F32LE", False), ("S24LE", "S24_32LE", False)):
        raw = stream(x, 2, 100, 5)
        got, pt = run(be, x, y, [raw])
        assert pt == expect, (x, y)
        if expect:
            same(got, [raw], (x, y))


def test_refusals_stay_refusals_on_host(emu_backend):
    check_refusals(emu_backend)


@pytest.mark.gpu
def test_refusals_stay_refusals_on_device(gpu_backend):
    check_refusals(gpu_backend)


# ---- the host's two loops agree ------------------------------------------------------------------------------------------------------
def test_sample_loop_and_lane_loop_agree_on_host(native_lib, emu_lib):
    """the emulator's older entry walks samples through the same unpack / pack bodies (and a per-sample form of the endian plan)"""
    lanes, single = EmuBackend(emu_lib), EmuBackend(emu_lib, "emu_aconv_")
    for ifmt, ofmt, cfg in (("S24BE", "S16BE", dict(dither_method="tpdf", noise_shaping="high")), ("F32LE", "U18BE", dict(dither_method="tpdf-hf")),
                            ("U20LE", "F64BE", {}), ("F32LE", "F32BE", dict(dither_method="tpdf")), ("S24BE", "S24LE", dict(noise_shaping="high")),
                            ("F64BE", "F64LE", {}), ("S16LE", "F32LE", {}), ("F32LE", "S24LE", dict(dither_method="rpdf"))):
        src = f32_specials() if ifmt == "F32LE" and ofmt == "F32BE" else None
        bufs = [src] if src is not None else [stream(ifmt, 2, n, n + 1) for n in (333, 64, 1)]
        same(run(single, ifmt, ofmt, bufs, **cfg)[0], run(lanes, ifmt, ofmt, bufs, **cfg)[0], (ifmt, ofmt, cfg))


# ---- 6. buffers that do not start on a dword ----------------------------------------------------------------------------------------
def check_alignment(be, offsets):
    """the four-sample lanes work on aligned dwords; whatever the buffers' addresses, the bytes are those of aligned buffers"""
    for ifmt, ofmt in (("S24BE", "S32LE"), ("S32LE", "S24BE"), ("S20LE", "F32LE"), ("F32LE", "U18BE"), ("S16BE", "F32LE"), ("F32LE", "U16BE"),
                       ("S24LE", "S24BE"), ("S16BE", "S16LE"), ("U8", "S16BE"), ("S16BE", "S8")):
        for n in (67, 5, 3):
            src = [stream(ifmt, 1, n, n)]
            exp, _ = run(be, ifmt, ofmt, src, in_ch=1, dither_method="tpdf")
            for io, oo in offsets:
                if io % min(BYTES[ifmt], 4) and BYTES[ifmt] != 3 or oo % min(BYTES[ofmt], 4) and BYTES[ofmt] != 3:
                    continue                    # buffers are aligned to their samples (3-byte samples have no alignment)
                got, _ = run(be, ifmt, ofmt, src, in_ch=1, dither_method="tpdf", in_off=io, out_off=oo)
                same(got, exp, (ifmt, ofmt, n, io, oo))


def test_unaligned_buffers_on_host(emu_backend):
    check_alignment(emu_backend, list(itertools.product(range(4), range(4))))


@pytest.mark.gpu
def test_unaligned_buffers_on_device(gpu_backend):
    check_alignment(gpu_backend, [(0, 0), (1, 0), (0, 1), (2, 2), (3, 1), (2, 0), (1, 3)])
