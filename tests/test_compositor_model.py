"""The compositor's kernels against tests/compositor_model.py - a numpy restatement of the blend semantics that needs no reference tree, so
nothing here skips where oracle/_ref is absent (but for the one test that pins the model to the reference the day the tree is back).

a. the model itself is pinned: to oracle/port.blend_a32 (which was pinned to the reference), to closed forms, and exhaustively for one pixel to
   a rational statement of the rule;
b. every scene of test_compositor.py / test_compositor_fuzz.py that takes `ref` runs again with the model in its place (the bodies are
   called as they stand, the parameter sets are the old tests' own marks).  Left out: the two 4K full-size scenes (workload size) and the
   scaled pads on the host emulator (they need the reference's converter; on the GPU the library's own golden-pinned converter stands in, so
   the expected canvas is the model's blend of that converter's output).  The fuzz scenes run ALL their seeds: with the model one seed of
   twelve scenes takes 0.02 - 0.05 s, kernels included (measured on an MI355X and on the host emulator);
c. edge scenes chosen from launch () and the kernel bodies, each on the host emulator (CPU) and through the C ABI (-m gpu).

The cases are the `check_*` functions with their parameter sets; a `test_*` function at the end of the file runs a group of them over all its cases and
reports every failing case.  One test per group, not one per case: the 1860 cases are cheap (a group takes a second or two), and the suite does not grow
by thousands of items.
"""
import ctypes as C
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest

import cases
import compositor_model as M
import test_compositor as TC
import test_compositor_fuzz as TF
from gstreamer_amd import video as V
from oracle import port

FMTS32 = ["BGRA", "RGBA", "VUYA", "ARGB", "ABGR", "AYUV"]
RUN_ARGS = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
CULL_ARGS = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
FRAME_ARGS = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]


class _LibraryConverter:
    """ref.VideoConverter's interface on the library's own converter (pinned to golden vectors elsewhere): GPU tests only"""

    def __init__(self, in_fmt, in_w, in_h, out_fmt, out_w, out_h, config=None):
        self.out_info = V.video_info(out_fmt, out_w, out_h)
        self.conv = V.VideoConverter(V.video_info(in_fmt, in_w, in_h), self.out_info,
                                     V.converter_config(resampler_method=config["GstVideoConverter__resampler_method"]))

    def frame(self, src):
        import torch
        d_src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8)).to("cuda:0")
        d = torch.zeros(int(self.out_info.size), dtype=torch.uint8, device="cuda:0")
        self.conv.frame(d_src, d)
        torch.cuda.synchronize()
        return d.cpu().numpy()


class _ModelAsRef:
    """the model where oracle/ref.py stands"""
    compositor_blend = staticmethod(M.compositor_blend)
    compositor_fill = staticmethod(M.compositor_fill)
    VideoConverter = _LibraryConverter

    @staticmethod
    def config_string(**opts):
        return opts


@pytest.fixture(scope="module")
def model():
    return _ModelAsRef


# ---- a. the model is itself pinned ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,alpha_byte", [("ARGB", 0), ("BGRA", 3)])
def check_model_opaque_blend_equals_the_oracle_port(fmt, alpha_byte):
    """oracle/port.blend_a32 was pinned to the reference's compositor_orc_blend_argb / _bgra while the tree was here"""
    func = "blend_" + TC.FAM[fmt]
    for i, (sw, sh, dw, dh, xpos, ypos, alpha) in enumerate([(37, 21, 64, 48, 5, 7, 0.5), (37, 21, 64, 48, -9, -4, 1.0), (100, 80, 64, 48, -20, -30, 0.3),
                                                             (10, 10, 64, 48, 70, 30, 0.7), (9, 9, 13, 7, 11, -8, 0.004), (9, 9, 13, 7, 1, 1, 0.0)]):
        src, dst = cases.frame_bytes(sw * sh * 4, "random", 40 + i), cases.frame_bytes(dw * dh * 4, "random", 60 + i)
        exp = port.blend_a32(src, sw, sh, xpos, ypos, alpha, dst.copy(), dw, dh, alpha_byte)
        for mode in (M.OVER, M.ADD):
            got = M.compositor_blend(func, fmt, src, sw, sh, xpos, ypos, alpha, dst.copy(), dw, dh, 0, dh, mode)
            assert (got == exp).all(), (i, mode)


@pytest.mark.parametrize("fmt", FMTS32)
def check_model_closed_forms(fmt):
    ab = M.ALPHA_BYTE[fmt]
    fam = TC.FAM[fmt]
    w, h = 23, 9
    src, dst = cases.frame_bytes(w * h * 4, "random", 71), cases.frame_bytes(w * h * 4, "random", 72)
    opaque = src.copy()
    opaque.reshape(-1, 4)[:, ab] = 255
    # an opaque pad at alpha 1.0 OVER gives the pad's pixel with alpha 0xff
    got = M.compositor_blend("blend_" + fam, fmt, opaque, w, h, 0, 0, 1.0, dst.copy(), w, h, 0, h, M.OVER)
    assert (got == opaque).all()
    # SOURCE at 1.0 is a copy, whatever the function
    for func in ("blend_", "overlay_"):
        assert (M.compositor_blend(func + fam, fmt, src, w, h, 0, 0, 1.0, dst.copy(), w, h, 0, h, M.SOURCE) == src).all()
    # overlay onto a zero canvas: the pad's colour with alpha `as` where as > 0, 0xff colour bytes with alpha 0 where as == 0
    some = src.copy()
    some.reshape(-1, 4)[::3, ab] = 0
    some.reshape(-1, 4)[1::3, ab] = 255
    for alpha in (1.0, 0.5, 0.004):
        sa = int(alpha * 255)
        got = M.compositor_blend("overlay_" + fam, fmt, some, w, h, 0, 0, alpha, np.zeros(w * h * 4, np.uint8), w, h, 0, h, M.OVER).reshape(-1, 4)
        a_s = some.reshape(-1, 4)[:, ab].astype(np.int64) * sa // 255
        exp = some.reshape(-1, 4).copy()
        exp[a_s == 0] = 255
        exp[:, ab] = a_s
        assert (got == exp).all(), alpha
        assert (a_s == 0).any() and (a_s > 0).any()
    # a pad alpha of 0 leaves the canvas alone
    for func in ("blend_", "overlay_"):
        for mode in (M.SOURCE, M.OVER, M.ADD):
            assert (M.compositor_blend(func + fam, fmt, src, w, h, 0, 0, 0.003, dst.copy(), w, h, 0, h, mode) == dst).all()


def check_model_plane_blend_closed_forms():
    d, s = np.arange(256, dtype=np.int64)[:, None], np.arange(256, dtype=np.int64)[None, :]
    assert (M._blend_u8(d, s, 0) == d).all()                         # a = 0 leaves d unchanged
    assert (M._blend_u8(d, d, 137) == d).all()                       # s == d: unchanged at any a
    for bits in (10, 12, 16):
        d16 = np.array([0, 1, 511, 1023, 4095, 32768, 65535], np.int64)[:, None]
        s16 = d16.T
        assert (M._blend_deep(d16, s16, 0, bits) == d16).all()
        assert (M._blend_deep(d16, d16 + 0 * s16, (1 << bits) - 1, bits) == d16).all()


def check_model_alpha_product_for_every_pair():
    """a = D (sA * s_alpha) for all 256 x 256 pairs: floor (sA * s_alpha / 255) as a rational, and the kernels' (x * 0x8081) >> 23"""
    sA, sa = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    a = M._d255(sA * sa)
    assert (a == ((sA * sa) * 0x8081) >> 23).all()
    for i in range(256):
        for j in range(256):
            assert int(a[i, j]) == math.floor(Fraction(i * j, 255))
    # D on every 16-bit x (the overlay's sums reach past 255 * 255)
    x = np.arange(65536, dtype=np.int64)
    assert (M._d255(x) == (x * 0x8081) >> 23).all()


def check_model_opaque_blend_for_every_byte_triple():
    """all (s, d, a): the model's pixel function against floor ((s * a + d * (255 - a)) / 255) - in exact 64-bit integers for all 2^24 triples, as
    Python rationals for 4096 of them.  With s_alpha = 255 the model's a is the source alpha byte itself (floor (sA * 255 / 255))."""
    s, d = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    rng = np.random.default_rng(5)
    for a in range(256):
        spx = np.stack([s, s, s, np.full_like(s, a)], axis=-1)
        dpx = np.stack([d, d, d, np.full_like(d, 77)], axis=-1)
        got = M.blend_px_a32(spx, dpx, 255, M.OVER, False, 3)
        exp = (s * a + d * (255 - a)) // 255
        assert (got[..., 0] == exp).all() and (got[..., 2] == exp).all() and (got[..., 3] == 255).all(), a
        for i, j in rng.integers(0, 256, (16, 2)):
            assert int(got[i, j, 1]) == math.floor(Fraction(int(i) * a + int(j) * (255 - a), 255))


def check_model_overlay_against_python_ints():
    """the overlay rule for random pixel pairs, restated per pixel with Python ints and floor divisions"""
    rng = np.random.default_rng(6)
    s, d = rng.integers(0, 256, (4000, 4)), rng.integers(0, 256, (4000, 4))
    s[::7, 0], d[::5, 0], s[::11, 0] = 0, 0, 255
    for sa in (255, 128, 1):
        for mode in (M.OVER, M.ADD):
            got = M.blend_px_a32(s.astype(np.int64), d.astype(np.int64), sa, mode, True, 0)
            for k in range(0, 4000, 9):
                sp, dp = [int(v) for v in s[k]], [int(v) for v in d[k]]
                a_s = sp[0] * sa // 255
                a_d = dp[0] * (255 - a_s) // 255
                n = (a_s + a_d) & 0xff
                exp = [255 if n == 0 else min(255, (sp[c] * a_s + dp[c] * a_d) // n) for c in range(4)]
                exp[0] = n if mode == M.OVER else (dp[0] + a_s) & 0xff
                assert [int(v) for v in got[k]] == exp, (sa, mode, k)


def check_model_wide64_against_python_ints():
    rng = np.random.default_rng(7)
    s, d = rng.integers(0, 65536, (3000, 4)), rng.integers(0, 65536, (3000, 4))
    s[::7, 0], d[::5, 0], s[::11, 0] = 0, 0, 65535
    for sa in (65535, 30000, 1):
        for mode in (M.SOURCE, M.OVER, M.ADD):
            for overlay in (False, True):
                got = M.blend_px_a64(s.astype(np.int64), d.astype(np.int64), sa, mode, overlay)
                for k in range(0, 3000, 13):
                    sp, dp = [int(v) for v in s[k]], [int(v) for v in d[k]]
                    a = min(65535, sp[0] * sa // 65535)
                    if mode == M.SOURCE:
                        exp = sp if sa == 65535 else [a] + sp[1:]
                    elif not overlay:
                        exp = [65535] + [min(65535, (sp[c] * a + dp[c] * (65535 - a)) // 65535) for c in (1, 2, 3)]
                    else:
                        da = dp[0] * (65535 - a) // 65535
                        fa = min(65535, da + a)
                        exp = [fa if mode == M.OVER else min(65535, dp[0] + a)]
                        exp += [min(65535, (dp[c] * da + sp[c] * a) // fa if fa else dp[c] * da + sp[c] * a) for c in (1, 2, 3)]
                    assert [int(v) for v in got[k]] == exp, (sa, mode, overlay, k)


@pytest.mark.parametrize("fmt", [f for f in TC.FRAME_FMTS if TC._frame_depth_shift(f)])
def check_model_deep_layout_equals_the_library(fmt):
    """two statements of gst_video_info_set_format's rule for the deep planar forms: either side being wrong shows"""
    for w, h in [(TC.FDW, TC.FDH), (5, 3), (1, 1), (2, 2), (64, 48)] + [p[:2] for p in TC.FRAME_PADS]:
        vi = V.video_info(fmt, w, h)
        assert ([int(vi.stride[i]) for i in range(3)], [int(vi.offset[i]) for i in range(3)], int(vi.size)) == M.deep_layout(fmt, w, h), (w, h)


def test_model_equals_the_reference(ref):
    """the day the reference tree is back: model == reference on every function and format (skips without oracle/_ref)"""
    sw, sh, dw, dh = 37, 21, 64, 48
    for fmt in FMTS32 + list(M.WIDE):
        wide = fmt in M.WIDE
        bpp, fam = (8, "argb64") if wide else (4, TC.FAM[fmt])
        for kind, fn, col in ((0, fmt.lower() if wide else TC.CHECKER_FN.get(fmt, fam), (0, 0, 0)), (1, "argb64" if wide else fmt.lower(), (10, 200, 77))):
            a, b = np.zeros(dw * dh * bpp, np.uint8), np.zeros(dw * dh * bpp, np.uint8)
            assert (ref.compositor_fill(kind, fn, fmt, a, dw, dh, 3, 40, *col) == M.compositor_fill(kind, fn, fmt, b, dw, dh, 3, 40, *col)).all(), (fmt, kind)
        for k, (func, mode, alpha, xpos, ypos) in enumerate((f + fam, m, al, x, y) for f in ("blend_", "overlay_") for m in (0, 1, 2)
                                                            for al in (1.0, 0.5, 0.004, 0.0) for x, y in ((5, 7), (-9, -4))):
            src, dst = cases.frame_bytes(sw * sh * bpp, "random", 300 + k), cases.frame_bytes(dw * dh * bpp, "random", 400 + k)
            if k % 3 == 0:
                src[0 if wide or M.ALPHA_BYTE[fmt] == 0 else 3::bpp][::4] = 0
                dst[0 if wide or M.ALPHA_BYTE[fmt] == 0 else 3::bpp][::3] = 0
            a = ref.compositor_blend(func, fmt, src, sw, sh, xpos, ypos, alpha, dst.copy(), dw, dh, 10, 40, mode)
            b = M.compositor_blend(func, fmt, src, sw, sh, xpos, ypos, alpha, dst.copy(), dw, dh, 10, 40, mode)
            assert (a == b).all(), (fmt, func, mode, alpha, xpos)
    for fmt in TC.FRAME_FMTS:
        for background in (0, 1, 2, 3):
            assert (TC._visible(fmt, TC._frame_expected(ref, fmt, background)) == TC._visible(fmt, TC._frame_expected(_ModelAsRef, fmt, background))).all(), (fmt, background)


# ---- b. the existing scenes with the model where `ref` stood ------------------------------------------------------------------------------------
LEFT_OUT = {"test_hip_aggregate_c4_full_size_matches_reference": "workload size (4K)", "test_hip_scaled_pads_c4_variant_a_full_size": "workload size (4K)",
            "test_scaled_pads_on_host_match_reference": "needs the reference's converter on the host"}


def _with_model(old):
    names = [n for n in inspect.signature(old).parameters if n != "ref"]

    def test(**kw):
        return old(ref=kw.pop("model"), **kw)
    test.__signature__ = inspect.Signature([inspect.Parameter(n, inspect.Parameter.POSITIONAL_OR_KEYWORD) for n in names + ["model"]])
    test.pytestmark = list(getattr(old, "pytestmark", []))          # the old test's own gpu mark and parameter sets
    test.__doc__ = old.__doc__
    return test


TWINS = {}          # old test name -> the same body with the model where `ref` stood
for _mod in (TC, TF):
    for _name, _fn in list(vars(_mod).items()):
        if _name.startswith("test_") and inspect.isfunction(_fn) and _fn.__module__ == _mod.__name__ and "ref" in inspect.signature(_fn).parameters \
                and _name not in LEFT_OUT:
            TWINS[_name] = _with_model(_fn)
            TWINS[_name].__name__ = "model_scene_" + _name[len("test_"):]


def _is_gpu(fn):
    return any(m.name == "gpu" for m in getattr(fn, "pytestmark", []))


# ---- c. edge scenes ---------------------------------------------------------------------------------------------------------------------------------
STALE = 0xa5
# the solid backgrounds in memory byte order, written out per format (the emulator takes the word; the library computes its own)
BG_BYTES = {("BGRA", 1): (0, 0, 0, 255), ("BGRA", 2): (255, 255, 255, 255), ("RGBA", 1): (0, 0, 0, 255), ("RGBA", 2): (255, 255, 255, 255),
            ("ARGB", 1): (255, 0, 0, 0), ("ARGB", 2): (255, 255, 255, 255), ("ABGR", 1): (255, 0, 0, 0), ("ABGR", 2): (255, 255, 255, 255),
            ("AYUV", 1): (255, 16, 128, 128), ("AYUV", 2): (255, 235, 128, 128), ("VUYA", 1): (128, 128, 16, 255), ("VUYA", 2): (128, 128, 235, 255)}
BG_WIDE = {("ARGB64", 1): (65535, 0, 0, 0), ("ARGB64", 2): (65535, 65535, 65535, 65535), ("AYUV64", 1): (65535, 4096, 32768, 32768),
           ("AYUV64", 2): (65535, 60160, 32768, 32768)}


class Pad:
    """one pad: `w` x `h` pixels of `bpp` bytes in a buffer of its own, rows `stride` bytes apart, the first `base` bytes into the buffer"""

    def __init__(self, w, h, x, y, alpha=1.0, mode=1, seed=0, pitch_extra=0, base=0, null=False, hint=None, bpp=4):
        self.w, self.h, self.x, self.y, self.alpha, self.mode, self.base, self.null, self.hint, self.bpp = w, h, x, y, alpha, mode, base, null, hint, bpp
        self.stride = w * bpp + pitch_extra
        self.buf = cases.frame_bytes(base + h * self.stride, "random", 1000 + seed)
        self.dev = None

    def rows(self):
        return self.buf[self.base:self.base + self.h * self.stride].reshape(self.h, self.stride)[:, :self.w * self.bpp]

    def px(self):
        """the pixels as a [h, w, bpp] view of the buffer"""
        return np.ndarray((self.h, self.w, self.bpp), np.uint8, self.buf, self.base, (self.stride, self.bpp, 1))

    def tight(self):
        return np.ascontiguousarray(self.rows()).reshape(-1)

    def host_ptr(self):
        return None if self.null else self.buf.ctypes.data + self.base

    def dev_ptr(self, gpu):
        import torch
        if self.null:
            return None
        if self.dev is None:
            self.dev = torch.from_numpy(self.buf).to(gpu)
        return self.dev.data_ptr() + self.base


def _set_alpha(pad, fmt, value, cols=None, rows=None):
    px = pad.px()
    px[slice(None) if rows is None else rows, slice(None) if cols is None else cols, M.ALPHA_BYTE[fmt]] = value


def model_canvas(fmt, background, pads, dw, dh, dstride):
    """the model's canvas: fill, then pad by pad; rows `dstride` apart with the bytes between them as they were (STALE)"""
    wide = fmt in M.WIDE
    bpp = 8 if wide else 4
    tight = np.zeros(dw * dh * bpp, np.uint8)
    if background == 0:
        M.compositor_fill(0, "checker", fmt, tight, dw, dh, 0, dh)
    elif background in (1, 2):
        yuv = "YUV" in fmt or fmt == "VUYA"
        sc = 256 if wide else 1
        col = (16 * sc, 128 * sc, 128 * sc) if yuv and background == 1 else (235 * sc, 128 * sc, 128 * sc) if yuv else ((0,) * 3 if background == 1 else (255 * sc + (255 if wide else 0),) * 3)
        M.compositor_fill(1, "color", fmt, tight, dw, dh, 0, dh, *col)
    func = ("overlay_" if background == 3 else "blend_") + ("argb64" if wide else TC.FAM[fmt])
    for p in pads:
        if not p.null:          # a pad without a frame is not drawn
            M.compositor_blend(func, fmt, p.tight(), p.w, p.h, p.x, p.y, p.alpha, tight, dw, dh, 0, dh, p.mode)
    full = np.full(dstride * dh, STALE, np.uint8)
    full.reshape(dh, dstride)[:, :dw * bpp] = tight.reshape(dh, dw * bpp)
    return full


def _fill_pad_dev(pd, p, sa):
    pd.data, pd.width, pd.height, pd.stride, pd.xpos, pd.ypos, pd.s_alpha, pd.mode = p.host_ptr(), p.w, p.h, p.stride, p.x, p.y, sa, p.mode


def emu_canvas(emu_lib, fmt, background, pads, dw, dh, dstride, hints=False):
    """the kernel bodies on the host, launched as aggregate_impl launches them: pads without alpha or frame dropped, 32 pads a launch, the launches after
    the first continue on the canvas (bg_kind 2), a launch with a usable hint takes the culling form"""
    emu_lib.emu_compositor_run.argtypes = RUN_ARGS
    emu_lib.emu_compositor_run_cull.argtypes = CULL_ARGS
    emu_lib.emu_compositor_wide64.argtypes = RUN_ARGS
    got = np.full(dstride * dh, STALE, np.uint8)
    wide = fmt in M.WIDE
    if wide:
        p = TC.Wide64Params()
        p.checker_yuv = int(fmt == "AYUV64")
        if background in (1, 2):
            p.bg_px = sum(v << (16 * k) for k, v in enumerate(BG_WIDE[fmt, background]))
    else:
        p = TC.AggParams()
        p.ashift = 0 if TC.FAM[fmt] == "argb" else 24
        p.checker_yuv = int(fmt in TC.CHECKER_FN)
        if background in (1, 2):
            p.bg_word = sum(v << (8 * k) for k, v in enumerate(BG_BYTES[fmt, background]))
    p.overlay, p.bg_kind = int(background == 3), (0 if background == 0 else 1)
    ash = M.ALPHA_BYTE.get(fmt, 0)
    done, first = 0, True
    while first or done < len(pads):
        k, maps, keep, all_bits, any_opaque = 0, (C.c_void_p * 32)(), [], 0, False
        while done < len(pads) and k < 32:
            pad = pads[done]
            done += 1
            sa = M.s_alpha_16(pad.alpha) if wide else M.s_alpha_8(pad.alpha)
            if sa == 0 or pad.null:
                continue
            if hints and sa == 255 and pad.hint:
                any_opaque = True
                if pad.hint == "all":
                    all_bits |= 1 << k
                else:
                    keep.append(TC._opacity_words(pad.tight(), pad.w, pad.h, ash))
                    maps[k] = keep[-1].ctypes.data
            _fill_pad_dev(p.pads[k], pad, sa)
            k += 1
        p.n_pads = k
        if wide:
            emu_lib.emu_compositor_wide64(C.byref(p), got.ctypes.data, dstride, 0, 0, dw, dh)
        elif any_opaque:
            emu_lib.emu_compositor_run_cull(C.byref(p), maps, all_bits, got.ctypes.data, dstride, 0, 0, dw, dh)
        else:
            emu_lib.emu_compositor_run(C.byref(p), got.ctypes.data, dstride, 0, 0, dw, dh)
        p.bg_kind, first = 2, False
    return got


def hip_canvas(gpu, fmt, background, pads, dw, dh, dstride, hints=False):
    import torch
    n = len(pads)
    arr, opa, hold = (V.CompositorPad * max(n, 1))(), (V.CompositorPadOpacity * max(n, 1))(), []
    ash = M.ALPHA_BYTE.get(fmt, 0)
    for i, p in enumerate(pads):
        arr[i].data, arr[i].width, arr[i].height, arr[i].stride = p.dev_ptr(gpu), p.w, p.h, p.stride
        arr[i].xpos, arr[i].ypos, arr[i].alpha, arr[i].blend_mode = p.x, p.y, p.alpha, p.mode
        if hints and p.hint == "all":
            opa[i].all_opaque = 1
        elif hints and p.hint == "map":
            m = torch.full((p.h,), -1, dtype=torch.int64, device=gpu)
            V._check(V.lib().gstamd_compositor_pad_opacity_map(V.FORMATS[fmt], p.dev_ptr(gpu), p.w, p.h, p.stride, m.data_ptr(), None))
            torch.cuda.synchronize()
            assert (m.cpu().numpy().view(np.uint64) == TC._opacity_words(p.tight(), p.w, p.h, ash)).all()
            hold.append(m)
            opa[i].map = m.data_ptr()
    d = torch.full((dstride * dh,), STALE, dtype=torch.uint8, device=gpu)
    if hints:
        V._check(V.lib().gstamd_compositor_aggregate_opaque(V.FORMATS[fmt], background, arr, opa, n, d.data_ptr(), dw, dh, dstride, None))
    else:
        V._check(V.lib().gstamd_compositor_aggregate(V.FORMATS[fmt], background, arr, n, d.data_ptr(), dw, dh, dstride, None))
    torch.cuda.synchronize()
    return d.cpu().numpy()


def _same(got, exp, what):
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (what, int(bad.size), [int(b) for b in bad[:8]])


# -- canvas widths and heights, pad geometry
EDGE_WIDTHS = [3, 4, 5, 203, 256, 257, 260, 517]
EDGE_HEIGHTS = [17, 33]


def edge_scene(dw, dh, variant):
    """pads for one canvas.  "fast": OVER / ADD pads of four pixels and more (k_aggregate_direct; k_aggregate where the canvas is narrower than four pixels).
    "mixed": the same with pads 1, 2 and 3 pixels wide and two SOURCE pads (k_aggregate's general form).  In both: a pad wider than the canvas, odd xpos,
    pad rows further apart than 4 * width, pad bases that are only 4-byte aligned, pads off the canvas on every side, a pad without a frame, pad alphas
    of 0.0, 0.003 (s_alpha 0) and 0.004 (s_alpha 1) in the middle of the list, pads over the right and the bottom edge"""
    pads = [Pad(dw + 9, 11, -5, -3, 0.6, 1, seed=1),
            Pad(7, 9, 1, 2, 1.0, 1, seed=2, pitch_extra=12, base=4),
            Pad(4, 5, dw - 3, dh - 3, 0.8, 2, seed=3),
            Pad(8, 8, dw, 0, 1.0, 1, seed=4), Pad(8, 8, -8, 3, 1.0, 1, seed=5), Pad(8, 8, 2, dh, 1.0, 1, seed=6), Pad(8, 8, 2, -8, 1.0, 1, seed=7),
            Pad(9, 9, 1, 1, 1.0, 1, seed=8, null=True),
            Pad(30, 12, 0, 4, 0.0, 1, seed=9), Pad(30, 12, 0, 4, 0.003, 1, seed=10), Pad(30, 12, 3, 5, 0.004, 2, seed=11),
            Pad(37, dh + 4, (dw // 2 - 11) | 1, -2, 0.45, 1, seed=12, pitch_extra=20, base=4),
            Pad(5, 3, -2, dh - 2, 0.9, 1, seed=13, base=8),
            Pad(64, 6, dw - 61, 9, 1.0, 2, seed=14),
            Pad(dw, 2, 0, dh - 5, 0.7, 1, seed=15)]
    if dw < 4:
        pads = [p for p in pads if p.w != dw] + [Pad(4, 2, 0, dh - 5, 0.7, 1, seed=15)]
    if variant == "mixed":
        pads[5:5] = [Pad(1, 7, 2, 3, 0.9, 1, seed=21), Pad(2, 7, dw - 1, 1, 0.8, 2, seed=22), Pad(3, 4, -1, 6, 1.0, 1, seed=23, base=4),
                     Pad(21, 10, 1, 0, 0.7, 0, seed=24, pitch_extra=8), Pad(6, 5, dw - 4, 12, 1.0, 0, seed=25)]
    return pads


def _edge_background(fmt, dw, dh, variant):
    k = FMTS32.index(fmt) + EDGE_WIDTHS.index(dw) + EDGE_HEIGHTS.index(dh)
    return k % 4 if variant == "mixed" else k % 3


def _edge_stride(dw):
    return 4 * dw + (32 if dw % 2 else 0)          # the odd widths: canvas rows further apart than 4 * width


EDGE_PARAMS = [(f, w, h, v) for f in FMTS32 for w in EDGE_WIDTHS for h in EDGE_HEIGHTS for v in ("fast", "mixed")]


@pytest.mark.parametrize("fmt,dw,dh,variant", EDGE_PARAMS)
def check_edge_canvases_on_host(emu_lib, fmt, dw, dh, variant):
    """widths: rw < 4 takes k_aggregate, a width that is no multiple of four moves the last lane back, 257 / 260 / 517 end in a short strip; heights 17 and 33:
    both checker phases in x and y; the bytes between the canvas rows stay as they were"""
    pads, bg, ds = edge_scene(dw, dh, variant), _edge_background(fmt, dw, dh, variant), _edge_stride(dw)
    emu_lib.emu_compositor_direct_runs.restype = C.c_int
    before = emu_lib.emu_compositor_direct_runs()
    got = emu_canvas(emu_lib, fmt, bg, pads, dw, dh, ds)
    assert emu_lib.emu_compositor_direct_runs() - before == int(variant == "fast" and dw >= 4)
    _same(got, model_canvas(fmt, bg, pads, dw, dh, ds), (fmt, dw, dh, variant, bg))


@pytest.mark.parametrize("fmt,dw,dh,variant", EDGE_PARAMS)
def check_hip_edge_canvases(native_lib, gpu, fmt, dw, dh, variant):
    pads, bg, ds = edge_scene(dw, dh, variant), _edge_background(fmt, dw, dh, variant), _edge_stride(dw)
    _same(hip_canvas(gpu, fmt, bg, pads, dw, dh, ds), model_canvas(fmt, bg, pads, dw, dh, ds), (fmt, dw, dh, variant, bg))


# -- more hits under one strip and row than request slots (AGG_DIRECT_SLOTS = 12)
def pile_scene(n):
    """n pads piled on rows 4 .. 10 around column 256: every one of them is a hit of both strips of those rows"""
    return [Pad(40 + i % 3, 9, 235 + (i % 5) * 2, 3 + i % 2, min(1.0, 0.25 + 0.02 * i), 1 if i % 3 else 2, seed=100 + i, base=4 * (i % 2)) for i in range(n)]


PILE_PARAMS = [(f, n) for f in FMTS32 for n in (12, 13, 29)]


@pytest.mark.parametrize("fmt,n", PILE_PARAMS)
def check_piled_pads_on_host(emu_lib, fmt, n):
    pads, bg = pile_scene(n), n % 3
    _same(emu_canvas(emu_lib, fmt, bg, pads, 300, 17, 1200), model_canvas(fmt, bg, pads, 300, 17, 1200), (fmt, n))


@pytest.mark.parametrize("fmt,n", PILE_PARAMS)
def check_hip_piled_pads(native_lib, gpu, fmt, n):
    pads, bg = pile_scene(n), n % 3
    _same(hip_canvas(gpu, fmt, bg, pads, 300, 17, 1200), model_canvas(fmt, bg, pads, 300, 17, 1200), (fmt, n))


# -- more pads than one launch takes (GSTAMD_MAX_FUSED_PADS = 32)
def many_scene(n, dw, dh, source):
    """`source`: pad 31, the last of the first launch, is a SOURCE pad at alpha 0.8 over most of the canvas (and pad 7 a small one that later pads cover) -
    it lowers the canvas alpha inside the first launch, and the continuation launches may force alpha only where their own pads are (the shape found
    late: more than 32 pads, a width that is no multiple of four)"""
    pads = [Pad(50, 12, (i * 37) % dw - 20, (i * 5) % dh - 4, min(1.0, 0.3 + 0.01 * i), 1 if i % 3 else 2, seed=200 + i) for i in range(n)]
    if source:
        pads[7] = Pad(60, 9, 30, 1, 0.8, 0, seed=298)
        pads[31] = Pad(dw - 40, dh - 2, 30, 1, 0.8, 0, seed=299)
        if n > 64:          # and the last pad of the second launch, for the third
            pads[63] = Pad(dw - 30, dh - 3, 3, 2, 0.9, 0, seed=297)
    return pads


def check_many_pads_scene_keeps_lowered_alpha_for_the_continuation():
    """the scene is the shape it claims to be: after all pads the model's canvas still holds pixels whose alpha the SOURCE pad lowered"""
    for n in (32, 33, 40, 65):
        for dw in (204, 203):
            a = model_canvas("BGRA", 0, many_scene(n, dw, 17, 1), dw, 17, 4 * dw).reshape(17, dw, 4)[:, :, 3]
            assert (a < 255).sum() > 100, (n, dw)


MANY_PARAMS = [(f, n, w, bg, s) for f in ("BGRA", "ARGB") for n in (32, 33, 40, 65) for w in (204, 203) for bg in (0, 1, 2, 3) for s in (0, 1)]


@pytest.mark.parametrize("fmt,n,dw,background,source", MANY_PARAMS)
def check_many_pads_on_host(emu_lib, fmt, n, dw, background, source):
    pads = many_scene(n, dw, 17, source)
    _same(emu_canvas(emu_lib, fmt, background, pads, dw, 17, 4 * dw), model_canvas(fmt, background, pads, dw, 17, 4 * dw), (fmt, n, dw, background, source))


@pytest.mark.parametrize("fmt,n,dw,background,source", MANY_PARAMS)
def check_hip_many_pads(native_lib, gpu, fmt, n, dw, background, source):
    pads = many_scene(n, dw, 17, source)
    _same(hip_canvas(gpu, fmt, background, pads, dw, 17, 4 * dw), model_canvas(fmt, background, pads, dw, 17, 4 * dw), (fmt, n, dw, background, source))


# -- row windows of the single-pad entries
WIN_DW, WIN_DH, WIN_GUARD = 37, 48, 8
WINDOWS = [(0, WIN_DH), (10, 40), (5, WIN_DH + 7)]
WINDOW_BLENDS = [(f, o, m, win) for f in FMTS32 for o, m in ((0, 1), (1, 1), (1, 2), (0, 0)) for win in WINDOWS]


def _window_blend_inputs(fmt, overlay, mode, win):
    k = FMTS32.index(fmt) * 16 + overlay * 8 + mode * 3 + WINDOWS.index(win)
    pad = Pad(29, 61, 11, -6, 0.7, mode, seed=400 + k, pitch_extra=4 * (k % 2))
    canvas = cases.frame_bytes(WIN_DW * (WIN_DH + WIN_GUARD) * 4, "random", 500 + k)          # WIN_GUARD rows behind the canvas: a window past dh must not reach them
    exp = canvas.copy()
    M.compositor_blend(("overlay_" if overlay else "blend_") + TC.FAM[fmt], fmt, pad.tight(), pad.w, pad.h, pad.x, pad.y, pad.alpha, exp[:WIN_DW * WIN_DH * 4],
                       WIN_DW, WIN_DH, win[0], win[1], mode)
    return pad, canvas, exp


@pytest.mark.parametrize("fmt,overlay,mode,win", WINDOW_BLENDS)
def check_blend_row_windows_on_host(emu_lib, fmt, overlay, mode, win):
    emu_lib.emu_compositor_run.argtypes = RUN_ARGS
    pad, got, exp = _window_blend_inputs(fmt, overlay, mode, win)
    p = TC.AggParams()
    p.ashift, p.overlay, p.bg_kind, p.n_pads = (0 if TC.FAM[fmt] == "argb" else 24), overlay, 2, 1
    _fill_pad_dev(p.pads[0], pad, M.s_alpha_8(pad.alpha))
    x0, r0, x1, r1 = max(pad.x, 0), max(pad.y, win[0]), min(pad.x + pad.w, WIN_DW), min(pad.y + pad.h, min(win[1], WIN_DH))     # gstamd_compositor_blend's rectangle
    emu_lib.emu_compositor_run(C.byref(p), got.ctypes.data, WIN_DW * 4, x0, r0, x1 - x0, r1 - r0)
    _same(got, exp, (fmt, overlay, mode, win))


@pytest.mark.parametrize("fmt,overlay,mode,win", WINDOW_BLENDS)
def check_hip_blend_row_windows(native_lib, gpu, fmt, overlay, mode, win):
    import torch
    pad, canvas, exp = _window_blend_inputs(fmt, overlay, mode, win)
    d = torch.from_numpy(canvas).to(gpu)
    V._check(V.lib().gstamd_compositor_blend(V.FORMATS[fmt], overlay, pad.dev_ptr(gpu), pad.w, pad.h, pad.stride, pad.x, pad.y, pad.alpha, d.data_ptr(),
                                              WIN_DW, WIN_DH, WIN_DW * 4, win[0], win[1], mode, None))
    torch.cuda.synchronize()
    _same(d.cpu().numpy(), exp, (fmt, overlay, mode, win))


def _window_fill_expected(fmt, kind, win):
    bpp = 8 if fmt in M.WIDE else 4
    canvas = cases.frame_bytes(WIN_DW * (WIN_DH + WIN_GUARD) * bpp, "random", 600)
    exp = canvas.copy()
    col = (4096, 51234, 777) if bpp == 8 else (10, 200, 77)
    M.compositor_fill(kind, "fill", fmt, exp[:WIN_DW * WIN_DH * bpp], WIN_DW, WIN_DH, win[0], win[1], *col)
    return canvas, exp, col


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("fmt", FMTS32 + list(M.WIDE))
def check_fill_row_windows_on_host(emu_lib, fmt, kind, win):
    """fill_checker / fill_color bodies over the rows [y0, min (y1, dh))"""
    emu_lib.emu_compositor_run.argtypes = emu_lib.emu_compositor_wide64.argtypes = RUN_ARGS
    got, exp, col = _window_fill_expected(fmt, kind, win)
    rows = min(win[1], WIN_DH) - win[0]
    if fmt in M.WIDE:
        p = TC.Wide64Params()
        p.bg_kind, p.checker_yuv, p.bg_px = kind, int(fmt == "AYUV64"), 0xffff | (col[0] << 16) | (col[1] << 32) | (col[2] << 48)
        emu_lib.emu_compositor_wide64(C.byref(p), got.ctypes.data, WIN_DW * 8, 0, win[0], WIN_DW, rows)
    else:
        p = TC.AggParams()
        p.ashift, p.bg_kind, p.checker_yuv = (0 if TC.FAM[fmt] == "argb" else 24), kind, int(fmt in TC.CHECKER_FN)
        p.bg_word = sum(v << (8 * k) for k, v in enumerate(M.color_bytes_a32(fmt, *col)))
        emu_lib.emu_compositor_run(C.byref(p), got.ctypes.data, WIN_DW * 4, 0, win[0], WIN_DW, rows)
    _same(got, exp, (fmt, kind, win))


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("fmt", FMTS32 + list(M.WIDE))
def check_hip_fill_row_windows(native_lib, gpu, fmt, kind, win):
    """gstamd_compositor_fill_checker / _fill_color: a window that reaches past the canvas ends at its last row (the rows behind it are not touched)"""
    import torch
    canvas, exp, col = _window_fill_expected(fmt, kind, win)
    bpp = 8 if fmt in M.WIDE else 4
    d = torch.from_numpy(canvas).to(gpu)
    if kind == 0:
        V._check(V.lib().gstamd_compositor_fill_checker(V.FORMATS[fmt], d.data_ptr(), WIN_DW, WIN_DH, WIN_DW * bpp, win[0], win[1], None))
    else:
        V._check(V.lib().gstamd_compositor_fill_color(V.FORMATS[fmt], d.data_ptr(), WIN_DW, WIN_DH, WIN_DW * bpp, win[0], win[1], *col, None))
    torch.cuda.synchronize()
    _same(d.cpu().numpy(), exp, (fmt, kind, win))


def check_fill_colour_words_written_out():
    """fill_color's bytes per format, written out by hand: what the model makes of (c1, c2, c3) = (10, 200, 77)"""
    assert {f: tuple(M.color_bytes_a32(f, 10, 200, 77)) for f in FMTS32} == {
        "ARGB": (255, 10, 200, 77), "AYUV": (255, 10, 200, 77), "BGRA": (77, 200, 10, 255), "VUYA": (77, 200, 10, 255), "ABGR": (255, 77, 200, 10),
        "RGBA": (10, 200, 77, 255)}
    for (fmt, bg), b in BG_BYTES.items():
        yuv = fmt in ("AYUV", "VUYA")
        col = ((16, 128, 128) if bg == 1 else (235, 128, 128)) if yuv else ((0,) * 3 if bg == 1 else (255,) * 3)
        assert tuple(M.color_bytes_a32(fmt, *col)) == b, (fmt, bg)


# -- opaque culling (gstamd_compositor_aggregate_opaque)
CULL_DW, CULL_DH = 600, 17          # strips [0, 256), [256, 512), [512, 600); an odd height against AGG_CULL_ROWS = 2


def cull_scene(fmt, extra):
    """pads with hints over a translucent base: all_opaque pads 63, 64, 65 and 300 pixels wide (the last covers the whole first strip), a mapped pad whose
    opaque run ends one pixel short of the first strip (and covers the second), a mapped pad at an xpos that is no multiple of 64, a flagged pad at pad alpha
    0.99 (the hint is ignored), a mapped pad opaque on alternate rows only, one whose first non-opaque block starts under the strip's last column, then
    pads on top.  `extra` small pads ahead of them push the hinted pads into the second and third launch."""
    pads = [Pad(30, 9, (i * 53) % CULL_DW - 7, (i * 3) % CULL_DH - 2, min(1.0, 0.35 + 0.01 * i), 1 if i % 4 else 2, seed=700 + i) for i in range(extra)]
    pads.append(Pad(CULL_DW, CULL_DH, 0, 0, 0.9, 1, seed=600))
    for k, (w, x, y) in enumerate([(63, 3, 1), (64, 90, 2), (65, 255, 0), (300, -20, 5)]):
        p = Pad(w, 8, x, y, 1.0, 1 if k % 2 else 2, seed=610 + k, hint="all")
        _set_alpha(p, fmt, 255)
        pads.append(p)
    short = Pad(CULL_DW, 9, 0, 8, 1.0, 1, seed=620, hint="map")
    _set_alpha(short, fmt, 255, cols=slice(0, 512))
    _set_alpha(short, fmt, 254, cols=255)
    pads.append(short)
    shifted = Pad(400, 7, -37, 3, 1.0, 1, seed=621, hint="map", pitch_extra=16)
    _set_alpha(shifted, fmt, 255)
    _set_alpha(shifted, fmt, 0, cols=399, rows=2)
    pads.append(shifted)
    ignored = Pad(CULL_DW, 3, 0, 12, 0.99, 1, seed=622, hint="all")
    _set_alpha(ignored, fmt, 255)
    pads.append(ignored)
    holes = Pad(520, 6, -4, 10, 1.0, 1, seed=623, hint="map")
    _set_alpha(holes, fmt, 255, rows=slice(0, 6, 2))
    pads.append(holes)
    # the strip's last column is the first pixel of a 64-pixel block that is not opaque: pad columns [1, 257) lie under the strip [0, 256)
    edge = Pad(330, 5, -1, 11, 1.0, 1, seed=624, hint="map")
    _set_alpha(edge, fmt, 255, cols=slice(0, 256))
    _set_alpha(edge, fmt, 7, cols=256)
    pads.append(edge)
    pads += [Pad(70, 20, 200, -2, 0.5, 1, seed=630), Pad(9, 9, 591, 8, 1.0, 2, seed=631)]
    return pads


CULL_PARAMS = [(f, bg, e) for f, bg in (("BGRA", 0), ("ARGB", 1), ("AYUV", 0), ("RGBA", 2), ("VUYA", 1), ("ABGR", 3)) for e in (0, 25, 60)]


@pytest.mark.parametrize("fmt,background,extra", CULL_PARAMS)
def check_opaque_hints_on_host(emu_lib, fmt, background, extra):
    pads = cull_scene(fmt, extra)
    emu_lib.emu_compositor_culled.restype = C.c_long
    before = emu_lib.emu_compositor_culled()
    got = emu_canvas(emu_lib, fmt, background, pads, CULL_DW, CULL_DH, 4 * CULL_DW, hints=True)
    assert (emu_lib.emu_compositor_culled() > before) == (background != 3)          # the transparent background takes the overlay functions: no culling
    _same(got, model_canvas(fmt, background, pads, CULL_DW, CULL_DH, 4 * CULL_DW), (fmt, background, extra))


@pytest.mark.parametrize("fmt,background,extra", CULL_PARAMS)
def check_hip_opaque_hints(native_lib, gpu, fmt, background, extra):
    pads = cull_scene(fmt, extra)
    _same(hip_canvas(gpu, fmt, background, pads, CULL_DW, CULL_DH, 4 * CULL_DW, hints=True), model_canvas(fmt, background, pads, CULL_DW, CULL_DH, 4 * CULL_DW),
          (fmt, background, extra))


def check_opacity_map_on_host_against_numpy(emu_lib):
    """bit b of a row's word = all (alpha == 255) over the pixels [64 b, 64 b + 64) of the row"""
    emu_lib.emu_compositor_opacity_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    for fmt in ("BGRA", "ARGB"):
        for p in cull_scene(fmt, 0):
            if p.hint:
                got = np.zeros(p.h, np.uint64)
                emu_lib.emu_compositor_opacity_map(p.host_ptr(), p.w, p.h, p.stride, 8 * M.ALPHA_BYTE[fmt], got.ctypes.data)
                a = p.px()[:, :, M.ALPHA_BYTE[fmt]]
                exp = [sum(int((a[y, 64 * b:64 * b + 64] == 255).all()) << b for b in range((p.w + 63) // 64)) for y in range(p.h)]
                assert [int(v) for v in got] == exp, (fmt, p.w)


# -- the plane formats (gstamd_compositor_aggregate_frame)
def frame_pads(n):
    """(w, h, xpos, ypos, alpha, mode): odd, even and negative positions, pads over every edge, every operator, pad alphas 0.0 / 0.004 / 0.996 / 1.0"""
    alphas, modes = [0.5, 1.0, 0.3, 0.0, 0.004, 0.996, 0.7], [1, 1, 0, 2, 1]
    return [(6 + (i * 7) % 31, 4 + (i * 5) % 23, (i * 13) % 111 - 9, (i * 11) % 75 - 5, alphas[i % 7], modes[i % 5]) for i in range(n)]


SMALL_PADS = [(3, 2, 1, 1, 0.5, 1), (4, 4, -1, -1, 0.7, 1), (2, 2, 3, 1, 1.0, 1), (1, 1, 4, 2, 0.3, 2), (6, 4, -3, 1, 0.6, 0)]
FRAME_SCENES = [(f, dw, dh, n) for f in TC.FRAME_FMTS for dw, dh, n in ((101, 67, 24), (101, 67, 25), (101, 67, 49), (5, 3, 0))]


def _frame_scene(fmt, dw, dh, n):
    pads = frame_pads(n) if n else SMALL_PADS
    srcs = [cases.frame_bytes(int(V.video_info(fmt, p[0], p[1]).size), "random", 7700 + k) for k, p in enumerate(pads)]
    return pads, srcs, (TC.FRAME_FMTS.index(fmt) + n) % 4


def frame_expected(fmt, background, pads, srcs, dw, dh):
    """TC._frame_expected for any canvas and pad list"""
    dst = cases.frame_bytes(int(V.video_info(fmt, dw, dh).size), "random", 6999)
    sh = TC._frame_depth_shift(fmt)
    if background == 0:
        M.compositor_fill(0, fmt.lower(), fmt, dst, dw, dh, 0, dh)
    elif background == 3 and sh:
        dst[:] = 0
    elif background == 3 and fmt in TC.FRAME_WHOLE:
        dst.reshape(dh, -1)[:, :dw * (2 if "Y" in fmt else 4)] = 0
    elif background == 3:
        strides, offsets = cases.default_layout(fmt, dw, dh)
        for i, (rb, rows) in enumerate(cases.visible_planes(fmt, dw, dh)):
            dst[offsets[i]:offsets[i] + strides[i] * rows].reshape(rows, strides[i])[:, :rb] = 0
    else:
        yuv = fmt not in TC.FRAME_RGB
        c = ((16, 128, 128) if yuv else (0, 0, 0)) if background == 1 else ((235, 128, 128) if yuv else (255, 255, 255))
        M.compositor_fill(1, fmt.lower(), fmt, dst, dw, dh, 0, dh, *[v << sh for v in c])
    for src, (w, h, x, y, alpha, mode) in zip(srcs, pads):
        M.compositor_blend("blend", fmt, src, w, h, x, y, alpha, dst, dw, dh, 0, dh, mode)
    return dst


def _frame_colours(fmt):
    yuv, sh = fmt not in TC.FRAME_RGB, TC._frame_depth_shift(fmt)
    return [v << sh for v in ((16, 128, 128) if yuv else (0, 0, 0))], [v << sh for v in ((235, 128, 128) if yuv else (255, 255, 255))]


@pytest.mark.parametrize("fmt,dw,dh,n", FRAME_SCENES)
def check_frame_canvases_on_host(emu_lib, fmt, dw, dh, n):
    """24, 25 and 49 pads (GSTAMD_PLANE_MAX_PADS = 24: one, two and three launches a plane) on the odd canvas 101 x 67, and a canvas of 5 x 3"""
    emu_lib.emu_compositor_aggregate_frame.argtypes = FRAME_ARGS
    pads, srcs, background = _frame_scene(fmt, dw, dh, n)
    arr = (TC.EmuFramePad * len(pads))()
    for k, (w, h, x, y, alpha, mode) in enumerate(pads):
        strides, offsets = TC._frame_layout(fmt, w, h)
        for i in range(len(strides)):
            arr[k].data[i], arr[k].stride[i] = srcs[k].ctypes.data + offsets[i], strides[i]
        arr[k].width, arr[k].height, arr[k].xpos, arr[k].ypos, arr[k].alpha, arr[k].mode = w, h, x, y, alpha, mode
    dst = cases.frame_bytes(int(V.video_info(fmt, dw, dh).size), "random", 6999)
    strides, offsets = TC._frame_layout(fmt, dw, dh)
    dp = (C.c_void_p * 3)(*[dst.ctypes.data + o for o in offsets] + [None] * (3 - len(offsets)))
    ds = (C.c_int * 3)(*strides + [0] * (3 - len(strides)))
    black, white = _frame_colours(fmt)
    assert emu_lib.emu_compositor_aggregate_frame(V.FORMATS[fmt], background, (C.c_int * 3)(*black), (C.c_int * 3)(*white), arr, len(pads), dp, ds, dw, dh) == 0
    exp = frame_expected(fmt, background, pads, srcs, dw, dh)
    _same(TC._frame_visible(fmt, dw, dh, dst), TC._frame_visible(fmt, dw, dh, exp), (fmt, dw, dh, n, background))


@pytest.mark.parametrize("fmt,dw,dh,n", FRAME_SCENES)
def check_hip_frame_canvases(native_lib, gpu, fmt, dw, dh, n):
    import torch
    pads, srcs, background = _frame_scene(fmt, dw, dh, n)
    d_srcs = [torch.from_numpy(s).to(gpu) for s in srcs]
    arr = (V.CompositorFramePad * len(pads))()
    for k, (w, h, x, y, alpha, mode) in enumerate(pads):
        strides, offsets = TC._frame_layout(fmt, w, h)
        for i in range(len(strides)):
            arr[k].data[i], arr[k].stride[i] = d_srcs[k].data_ptr() + offsets[i], strides[i]
        arr[k].width, arr[k].height, arr[k].xpos, arr[k].ypos, arr[k].alpha, arr[k].blend_mode = w, h, x, y, alpha, mode
    d = torch.from_numpy(cases.frame_bytes(int(V.video_info(fmt, dw, dh).size), "random", 6999)).to(gpu)
    strides, offsets = TC._frame_layout(fmt, dw, dh)
    dp = (C.c_void_p * 3)(*[d.data_ptr() + o for o in offsets] + [None] * (3 - len(offsets)))
    ds = (C.c_int32 * 3)(*strides + [0] * (3 - len(strides)))
    V._check(V.lib().gstamd_compositor_aggregate_frame(V.FORMATS[fmt], background, None, None, arr, len(pads), dp, ds, dw, dh, None))
    torch.cuda.synchronize()
    exp = frame_expected(fmt, background, pads, srcs, dw, dh)
    _same(TC._frame_visible(fmt, dw, dh, d.cpu().numpy()), TC._frame_visible(fmt, dw, dh, exp), (fmt, dw, dh, n, background))


def check_deep_planes_meet_the_32_bit_wrap():
    """the deep formats are fed full-range 16-bit random samples (the frames above).  What the model's deep blend meets on them: the product (s - d) * a wraps
    modulo 2^32 wherever s < d, and samples above the nominal 2^bits - 1 pass through.  The saturation of the rule's last step cannot trigger: with
    0 <= a < 2^bits the sum is d * (2^bits - a) + s * a <= 65535 * 2^bits, never negative, so t <= 65535 for any 16-bit s and d - the model counts it, and
    the count is 0 (M._blend_deep)."""
    for fmt in ("I420_10LE", "I422_12LE", "Y444_16LE"):
        for k in M.stats:
            M.stats[k] = 0
        pads, srcs, _bg = _frame_scene(fmt, 101, 67, 25)
        frame_expected(fmt, 0, pads, srcs, 101, 67)
        assert M.stats["wrapped"] > 0, fmt
        assert M.stats["above_nominal"] > 0 or fmt == "Y444_16LE", fmt
        assert M.stats["saturated"] == 0, fmt


# -- ARGB64 / AYUV64
def wide_scene():
    pads = [Pad(20 + i % 7, 8 + i % 5, (i * 17) % 67 - 9, (i * 5) % 19 - 3, [1.0, 0.6, 0.3, 0.00002, 0.0][i % 5], i % 3, seed=800 + i, bpp=8, pitch_extra=8 * (i % 2)) for i in range(33)]
    for p in pads[::4]:          # transparent and opaque source pixels: the overlay's "final alpha 0" branch
        p.px()[:, 0::3, 0:2] = 0
        p.px()[:, 1::3, 0:2] = 255
    return pads


WIDE_PARAMS = [(f, bg) for f in M.WIDE for bg in (0, 1, 2, 3)]


@pytest.mark.parametrize("fmt,background", WIDE_PARAMS)
def check_wide64_canvases_on_host(emu_lib, fmt, background):
    """the three operators, 33 pads (two launches), every background; canvas rows further apart than 8 * width"""
    assert C.sizeof(TC.Wide64Params) == emu_lib.emu_sizeof_wide64()
    pads = wide_scene()
    _same(emu_canvas(emu_lib, fmt, background, pads, 67, 19, 67 * 8 + 16), model_canvas(fmt, background, pads, 67, 19, 67 * 8 + 16), (fmt, background))


@pytest.mark.parametrize("fmt,background", WIDE_PARAMS)
def check_hip_wide64_canvases(native_lib, gpu, fmt, background):
    pads = wide_scene()
    _same(hip_canvas(gpu, fmt, background, pads, 67, 19, 67 * 8 + 16), model_canvas(fmt, background, pads, 67, 19, 67 * 8 + 16), (fmt, background))


# ---- the tests: each runs a group of the checks above over all their parameter sets and reports every failing case --------------------------------
# (one test per group and not one per case: the cases are cheap - a group takes seconds - and the suite's run stays short of thousands of further items)
def _cases_of(fn):
    """the parameter sets of a function's own parametrize marks, as keyword dictionaries"""
    sets = [{}]
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        grown = []
        for base in sets:
            for v in m.args[1]:
                v = getattr(v, "values", v)
                grown.append(dict(base, **dict(zip(names, v if len(names) > 1 else (v,)))))
        sets = grown
    return sets


def _run_group(fns, **fixtures):
    failures, n = [], 0
    for fn in fns:
        wanted = inspect.signature(fn).parameters
        for case in _cases_of(fn):
            kw = dict({k: v for k, v in fixtures.items() if k in wanted}, **case)
            with pytest.MonkeyPatch.context() as mp:          # a case's environment ends with the case
                if "monkeypatch" in wanted:
                    kw["monkeypatch"] = mp
                n += 1
                try:
                    fn(**kw)
                except Exception as e:          # noqa: BLE001 - every failing case is reported, not the first
                    failures.append("%s%r: %s: %s" % (fn.__name__, tuple(str(v)[:40] for v in case.values()), type(e).__name__, str(e)[:300]))
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), n, "\n".join(failures[:40]))
    return n


def _model_is_pinned():
    """a: the oracle port, the closed forms, every (sA, s_alpha) pair and (s, d, a) triple, the overlay and 64-bit rules in Python ints, the deep layout"""
    n = _run_group([check_model_opaque_blend_equals_the_oracle_port, check_model_closed_forms, check_model_plane_blend_closed_forms,
                    check_model_alpha_product_for_every_pair, check_model_opaque_blend_for_every_byte_triple, check_model_overlay_against_python_ints,
                    check_model_wide64_against_python_ints, check_model_deep_layout_equals_the_library, check_fill_colour_words_written_out,
                    check_many_pads_scene_keeps_lowered_alpha_for_the_continuation, check_deep_planes_meet_the_32_bit_wrap])
    assert n == 2 + 6 + 7 + 8


def _reference_scenes_on_host_against_the_model(emu_lib, model):
    """b: every host test of test_compositor.py / test_compositor_fuzz.py that takes `ref`, over its own parameter sets"""
    assert len(TWINS) == 29 - len(LEFT_OUT)
    host = [f for name, f in TWINS.items() if not _is_gpu(f)]
    assert len(host) == 10
    assert _run_group(host, emu_lib=emu_lib, model=model) == 281 - 14         # the 281 cases that skip without the reference, less the host scaled-pad ones


@pytest.mark.gpu
def test_hip_reference_scenes_against_the_model(native_lib, gpu, model):
    """b: every `gpu` test of the two files that takes `ref` (but the two 4K scenes), over its own parameter sets and all fuzz seeds"""
    dev = [f for name, f in TWINS.items() if _is_gpu(f)]
    assert len(dev) == 16
    assert _run_group(dev, native_lib=native_lib, gpu=gpu, model=model) == 423


def _edge_scenes_on_host(emu_lib):
    """c: canvas widths and heights, pad geometry, piled pads, more pads than a launch takes; the bodies of gstamd_compositor_blend, fill_checker and
    fill_color over the row windows (0, dh), (10, 40), (5, dh + 7); k_aggregate_direct_cull's body with all_opaque and mapped pads, the map against
    numpy; the plane formats (24 / 25 / 49 pads, 101 x 67 and 5 x 3 canvases); ARGB64 / AYUV64 (three operators, four backgrounds, 33 pads)"""
    n = _run_group([check_edge_canvases_on_host, check_piled_pads_on_host, check_many_pads_on_host, check_blend_row_windows_on_host,
                    check_fill_row_windows_on_host, check_opaque_hints_on_host, check_opacity_map_on_host_against_numpy, check_frame_canvases_on_host,
                    check_wide64_canvases_on_host], emu_lib=emu_lib)
    assert n == 338 + 120 + 18 + 1 + 96


@pytest.mark.gpu
def test_hip_edge_scenes(native_lib, gpu):
    """c: the same scenes through the C ABI"""
    n = _run_group([check_hip_edge_canvases, check_hip_piled_pads, check_hip_many_pads, check_hip_blend_row_windows, check_hip_fill_row_windows,
                    check_hip_opaque_hints, check_hip_frame_canvases, check_hip_wide64_canvases], native_lib=native_lib, gpu=gpu)
    assert n == 338 + 120 + 18 + 96


def test_compositor_on_host_against_the_model(emu_lib, model):
    """a, b and c on the host: the model's own pins, the old host scenes with the model where `ref` stood, the edge scenes on the emulator - one item
    of the suite; a failure names the part and every failing case"""
    failures = []
    for part, args in ((_model_is_pinned, ()), (_reference_scenes_on_host_against_the_model, (emu_lib, model)), (_edge_scenes_on_host, (emu_lib,))):
        try:
            part(*args)
        except AssertionError as e:
            failures.append("%s: %s" % (part.__name__, e))
    assert not failures, "\n".join(failures)
