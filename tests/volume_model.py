"""The volume element's arithmetic as numpy: the tables of DESIGN 3.10.1, (a) a fixed volume and (b) per-frame gains, restated from the
document alone - int64 for the integer arithmetic, element-wise float32 / float64 products, ORC's denormal flush with bit masks.  It
imports nothing from gstreamer_amd/csrc and does not call the emulator.  tests/test_volume.py compares the product with it byte for
byte, and checks it against the stock `volume` element where that is installed.

Samples are flat numpy arrays of DT[fmt]; S24LE samples are int32 values in -2^23 .. 2^23 - 1, turned into their three bytes by
to_bytes."""
import numpy as np

DT = {"S8": np.int8, "S16LE": np.int16, "S24LE": np.int32, "S32LE": np.int32, "F32LE": np.float32, "F64LE": np.float64}
FORMATS = list(DT)
BITS = {"S8": 8, "S16LE": 16, "S24LE": 24, "S32LE": 32}
SHIFT = {"S8": 3, "S16LE": 11, "S24LE": 19, "S32LE": 27}         # the integer volume is (int) (vf * 2^SHIFT)
BPS = {"S8": 1, "S16LE": 2, "S24LE": 3, "S32LE": 4, "F32LE": 4, "F64LE": 8}
PIECE = {"S8": 16, "S16LE": 8, "S24LE": 4, "S32LE": 4, "F32LE": 4, "F64LE": 2}        # samples a lane owns


def to_bytes(fmt, a):
    a = np.ascontiguousarray(a, DT[fmt])
    if fmt != "S24LE":
        return a.view(np.uint8).copy()
    return a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()


def from_bytes(fmt, b):
    b = np.ascontiguousarray(b, np.uint8)
    if fmt != "S24LE":
        return b.view(DT[fmt]).copy()
    w = np.zeros((b.size // 3, 4), np.uint8)
    w[:, :3] = b.reshape(-1, 3)
    return (w.view("<u4").reshape(-1).astype(np.int64) << 40 >> 40).astype(np.int32)         # sign-extended from 24 bits


def fl(x):
    """ORC's denormal flush: a value whose exponent field is zero keeps only its sign bit"""
    if x.dtype == np.float32:
        b = x.view(np.uint32)
        return np.where((b & np.uint32(0x7f800000)) == 0, b & np.uint32(0xff800000), b).view(np.float32)
    b = x.view(np.uint64)
    return np.where((b & np.uint64(0x7ff0000000000000)) == 0, b & np.uint64(0xfff0000000000000), b).view(np.float64)


def sat(fmt, t):
    """satN of an int64 (or an already truncated float) array"""
    bits = BITS[fmt]
    return np.clip(t, -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(DT[fmt])


def held(volume, as_type=np.float32):
    """vf: the element holds its volume as a float (as_type = float64: the wrong model the tests tell apart from the right one)"""
    return float(as_type(volume))


def fixed_kind(volume, mute, as_type=np.float32):
    """'silence', 'pass' or 'scale', in the order of rule (a)"""
    vf = held(volume, as_type)
    if mute or vf == 0.0:
        return "silence"
    return "pass" if int(vf * 2048.0) == 2048 else "scale"


def fixed(fmt, s, volume, mute=False, as_type=np.float32):
    """rule (a)"""
    s = np.ascontiguousarray(s, DT[fmt])
    kind = fixed_kind(volume, mute, as_type)
    if kind == "silence":
        return np.zeros(s.size, DT[fmt])
    if kind == "pass":
        return s.copy()
    vf = held(volume, as_type)
    if fmt in BITS:
        v = int(vf * float(1 << SHIFT[fmt]))            # truncation
        return sat(fmt, (s.astype(np.int64) * v) >> SHIFT[fmt])
    with np.errstate(all="ignore"):
        v = fl(np.array([vf]).astype(DT[fmt]))[0]       # (float) vf for F32, vf for F64
        return fl(fl(s) * v)


def uses_doubles(fmt, ch):
    """rule (b): the rows that are the reference's plain C loops"""
    if fmt in ("S24LE", "S32LE"):
        return True
    return ch >= 2 if fmt == "F64LE" else ch >= 3


def gains(fmt, ch, s, g, mute=False, doubles=None):
    """rule (b): g one double per frame; doubles: None for the channel rule, True / False to force a row"""
    s = np.ascontiguousarray(s, DT[fmt])
    g = np.ascontiguousarray(g, np.float64)
    assert s.size == g.size * ch
    if mute:
        g = np.zeros(g.size, np.float64)
    gs = np.repeat(g, ch)
    if doubles is None:
        doubles = uses_doubles(fmt, ch)
    with np.errstate(all="ignore"):
        if fmt in BITS:
            if doubles:
                return sat(fmt, np.trunc(s.astype(np.float64) * gs))
            return sat(fmt, np.trunc(fl(s.astype(np.float32) * fl(gs.astype(np.float32))).astype(np.float64)))
        if fmt == "F32LE":
            if doubles:
                return (s.astype(np.float64) * gs).astype(np.float32)       # plain IEEE, denormals kept
            return fl(fl(s) * fl(gs.astype(np.float32)))
        if doubles:
            return s * gs                                                   # plain IEEE
        return fl(fl(s) * fl(gs))
