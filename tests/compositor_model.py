"""tests/compositor_model.py - the compositor's semantics restated in numpy integer arithmetic (TEST INFRASTRUCTURE ONLY).

It stands wherever oracle/ref.py's `compositor_blend` / `compositor_fill` stand (same signatures) and needs no reference tree.  It imports
numpy and, for the 8-bit buffer layouts, tests/cases.py - nothing of the product, the oracle or the host emulator.

Shape: the canvas is filled, then ONE PAD AFTER ANOTHER updates a clipped rectangle of the whole canvas, vectorised per rectangle.  The
kernels go the other way round (one output pixel gathers its pads), so the two do not share a mistake easily.  The rules are those listed
in the kernels' headers (compositor_device.h, compositor_wide.h, compositor_planes.h), written with plain `// 255`, `// norm` and explicit
16-bit masks; tests/test_compositor_model.py pins them to oracle/port.blend_a32, to closed forms and exhaustively to rational statements.

`stats` counts what the deep-plane blend met (see _blend_deep); the tests read it.
"""
import numpy as np

import cases

SOURCE, OVER, ADD = 0, 1, 2

# memory byte of alpha in the 32-bit formats with per-pixel alpha
ALPHA_BYTE = {"BGRA": 3, "RGBA": 3, "VUYA": 3, "ARGB": 0, "ABGR": 0, "AYUV": 0}
WIDE = ("ARGB64", "AYUV64")
# fill_color: shifts (A, C1, C2, C3) of the big-endian word
COLOR_SHIFTS = {"ARGB": (24, 16, 8, 0), "AYUV": (24, 16, 8, 0), "BGRA": (0, 8, 16, 24), "VUYA": (0, 8, 16, 24), "ABGR": (24, 0, 8, 16),
                "RGBA": (0, 24, 16, 8)}

stats = {"wrapped": 0, "saturated": 0, "above_nominal": 0}


def _m16(x):
    return x & 0xffff


def _d255(x):
    """D(x) = (x & 0xffff) // 255"""
    return _m16(x) // 255


def s_alpha_8(alpha):
    return min(max(int(alpha * 255), 0), 255)


def s_alpha_16(alpha):
    return min(max(int(alpha * 65535), 0), 65535)


def _clip(sw, sh, xpos, ypos, dw, dh, y0, y1):
    """the pad intersected with the canvas columns and the rows [y0, min(y1, dh)): (x0, x1, r0, r1) or None"""
    x0, x1 = max(xpos, 0), min(xpos + sw, dw)
    r0, r1 = max(ypos, y0), min(ypos + sh, min(y1, dh))
    if x1 <= x0 or r1 <= r0:
        return None
    return x0, x1, r0, r1


# ---- 32-bit formats with alpha ---------------------------------------------------------------------------------------------------------
def blend_px_a32(s, d, s_alpha, mode, overlay, ab):
    """one pad on pixels: s, d int64 arrays [..., 4] in memory byte order; returns the new destination pixels"""
    sA = s[..., ab:ab + 1]
    if mode == SOURCE:
        out = s.copy()
        if s_alpha != 255:
            out[..., ab] = _d255(sA * s_alpha)[..., 0] & 0xff
        return out
    if not overlay:
        a = _d255(sA * s_alpha)
        out = _d255(_m16(s * a) + _m16(d * _m16(255 - a))) & 0xff
        out[..., ab] = 0xff
        return out
    dA = d[..., ab:ab + 1]
    a_s = _d255(sA * s_alpha)
    a_d = _d255(dA * _m16(255 - a_s))
    n = (a_s + a_d) & 0xff
    total = _m16(_m16(s * a_s) + _m16(d * a_d))
    out = np.where(n == 0, 255, np.minimum(255, total // np.maximum(n, 1)))
    out[..., ab] = (n if mode == OVER else (dA + a_s) & 0xff)[..., 0]
    return out


def _blend_a32(func, fmt, src, sw, sh, xpos, ypos, alpha, dst, dw, dh, y0, y1, mode):
    ab = ALPHA_BYTE[fmt]
    assert func.endswith("argb" if ab == 0 else "bgra"), (func, fmt)
    sa = s_alpha_8(alpha)
    if sa == 0:
        return dst
    box = _clip(sw, sh, xpos, ypos, dw, dh, y0, y1)
    if box is None:
        return dst
    x0, x1, r0, r1 = box
    s = src[:sw * sh * 4].reshape(sh, sw, 4)[r0 - ypos:r1 - ypos, x0 - xpos:x1 - xpos].astype(np.int64)
    view = dst[:dw * dh * 4].reshape(dh, dw, 4)[r0:r1, x0:x1]
    view[...] = blend_px_a32(s, view.astype(np.int64), sa, mode, func.startswith("overlay_"), ab).astype(np.uint8)
    return dst


def checker_value(x, y):
    """80 / 160 in 8 x 8 squares: 160 where exactly one of (x >> 3) & 1, (y >> 3) & 1 is set"""
    return np.where((((x >> 3) & 1) + ((y >> 3) & 1)) == 1, 160, 80)


def _checker_grid(w, rows):
    y, x = np.meshgrid(np.asarray(rows), np.arange(w), indexing="ij")
    return checker_value(x, y)


def color_bytes_a32(fmt, c1, c2, c3):
    """the four memory bytes of the big-endian word (0xff << A) | (c1 << C1) | (c2 << C2) | (c3 << C3)"""
    A, C1, C2, C3 = COLOR_SHIFTS[fmt]
    word = (0xff << A) | (c1 << C1) | (c2 << C2) | (c3 << C3)
    return [(word >> sh) & 0xff for sh in (24, 16, 8, 0)]


def _fill_a32(kind, fmt, dst, dw, dh, y0, y1, c1, c2, c3):
    rows = np.arange(y0, min(y1, dh))
    if rows.size == 0:
        return dst
    view = dst[:dw * dh * 4].reshape(dh, dw, 4)
    if kind == 0:
        v = _checker_grid(dw, rows)
        ab = ALPHA_BYTE[fmt]
        px = np.empty((rows.size, dw, 4), np.int64)
        if fmt in ("AYUV", "VUYA"):
            px[...] = 128
            px[..., 1 if fmt == "AYUV" else 2] = v
        else:
            px[...] = v[..., None]
        px[..., ab] = 255
        view[rows] = px.astype(np.uint8)
    else:
        view[rows] = np.array(color_bytes_a32(fmt, c1, c2, c3), np.uint8)
    return dst


# ---- ARGB64 / AYUV64: 16-bit little-endian components, alpha first ---------------------------------------------------------------------------
def blend_px_a64(s, d, s_alpha, mode, overlay):
    """s, d: int64 arrays [..., 4] of 16-bit components (alpha first); every quotient clamped to 65535"""
    q = lambda x: np.minimum(x, 65535)
    sA = s[..., 0:1]
    if mode == SOURCE:
        out = s.copy()
        if s_alpha != 65535:
            out[..., 0] = q(sA * s_alpha // 65535)[..., 0]
        return out
    sa = q(sA * s_alpha // 65535)
    if not overlay:
        out = q((s * sa + d * (65535 - sa)) // 65535)
        out[..., 0] = 65535
        return out
    dA = d[..., 0:1]
    da = q(dA * (65535 - sa) // 65535)
    fa = q(da + sa)
    c = d * da + s * sa
    out = q(np.where(fa > 0, c // np.maximum(fa, 1), c))
    out[..., 0] = (fa if mode == OVER else q(dA + sa))[..., 0]
    return out


def _blend_a64(func, fmt, src, sw, sh, xpos, ypos, alpha, dst, dw, dh, y0, y1, mode):
    sa = s_alpha_16(alpha)
    if sa == 0:
        return dst
    box = _clip(sw, sh, xpos, ypos, dw, dh, y0, y1)
    if box is None:
        return dst
    x0, x1, r0, r1 = box
    s = src[:sw * sh * 8].view("<u2").reshape(sh, sw, 4)[r0 - ypos:r1 - ypos, x0 - xpos:x1 - xpos].astype(np.int64)
    view = dst[:dw * dh * 8].view("<u2").reshape(dh, dw, 4)[r0:r1, x0:x1]
    view[...] = blend_px_a64(s, view.astype(np.int64), sa, mode, func.startswith("overlay_")).astype(np.uint16)
    return dst


def _fill_a64(kind, fmt, dst, dw, dh, y0, y1, c1, c2, c3):
    rows = np.arange(y0, min(y1, dh))
    if rows.size == 0:
        return dst
    view = dst[:dw * dh * 8].view("<u2").reshape(dh, dw, 4)
    if kind == 0:
        v = _checker_grid(dw, rows) * 256               # 20480 / 40960
        px = np.empty((rows.size, dw, 4), np.int64)
        px[...] = 32768 if fmt == "AYUV64" else v[..., None]
        px[..., 1] = v
        px[..., 0] = 65535
        view[rows] = px.astype(np.uint16)
    else:
        view[rows] = np.array([65535, c1, c2, c3], np.uint16)
    return dst


# ---- formats without per-pixel alpha: plane by plane, pad alpha only ----------------------------------------------------------------------
PACKED_422 = {"YUY2": (0, 1, 3), "UYVY": (1, 0, 2), "YVYU": (0, 3, 1)}          # byte of Y0 (Y1 = Y0 + 2), U, V in the macropixel
RGB3 = {"RGB": (0, 1, 2), "BGR": (2, 1, 0)}                                      # byte of R, G, B
XRGB4 = {"xRGB": (0, (1, 2, 3)), "xBGR": (0, (3, 2, 1)), "RGBx": (3, (0, 1, 2)), "BGRx": (3, (2, 1, 0))}      # x byte, bytes of R, G, B


def depth_bits(fmt):
    return 10 if "_10" in fmt else 12 if "_12" in fmt else 16 if "_16" in fmt else 8


def plane_geometry(fmt):
    """(planes [(w_sub, h_sub, bytes per subsampled pixel)], x positions round to even, y positions round to even)"""
    base = fmt.split("_")[0]
    sb = 2 if depth_bits(fmt) > 8 else 1
    if base in ("I420", "YV12"):
        return [(0, 0, sb), (1, 1, sb), (1, 1, sb)], True, True
    if base in ("Y42B", "I422"):
        return [(0, 0, sb), (1, 0, sb), (1, 0, sb)], True, False
    if base == "Y444":
        return [(0, 0, sb)] * 3, False, False
    if base in ("NV12", "NV21"):
        return [(0, 0, 1), (1, 1, 2)], True, True
    if base in RGB3:
        return [(0, 0, 3)], False, False
    if base in XRGB4:
        return [(0, 0, 4)], False, False
    if base in PACKED_422:
        return [(0, 0, 2)], True, False
    raise ValueError(fmt)


def _up(v, sub):
    return -((-v) >> sub)


def deep_layout(fmt, w, h):
    """(strides, offsets, size) of the 10 / 12 / 16-bit planar forms: strides rounded up to 4 bytes, chroma sizes by rounding up, planes of an
    even number of luma rows where a plane is subsampled"""
    r4 = lambda v: (v + 3) // 4 * 4
    r2 = lambda v: (v + 1) // 2 * 2
    planes, _x, _y = plane_geometry(fmt)
    sub_h = planes[1][1]
    sub_any = planes[1][0] or planes[1][1]
    strides = [r4(2 * w)] + [r4(2 * _up(r2(w), pl[0])) for pl in planes[1:]]
    hh = r2(h) if sub_any else h
    o1 = strides[0] * hh
    o2 = o1 + strides[1] * (hh >> sub_h)
    return strides, [0, o1, o2], o2 + strides[2] * (hh >> sub_h)


def frame_layout(fmt, w, h):
    if depth_bits(fmt) > 8:
        return deep_layout(fmt, w, h)[:2]
    return cases.default_layout(fmt, w, h)


def _plane_view(buf, stride, offset, rows):
    return buf[offset:offset + stride * rows].reshape(rows, stride)


def _blend_u8(d, s, a):
    """d = ((d << 8) + (s - d) * a) >> 8, kept to 8 bits"""
    return (((d << 8) + (s - d) * a) >> 8) & 0xff


def _blend_deep(d, s, a, bits):
    """t = ((d << bits) + (s - d) * a) mod 2^32 >> bits, read as signed 32-bit and saturated to [0, 65535].

    With 0 <= a < 2^bits the sum is d * (2^bits - a) + s * a: never negative and never above 65535 << bits, so the saturation cannot trigger on
    16-bit samples (stats["saturated"] counts it all the same); what does happen is the 32-bit wrap of the negative product (s - d) * a, which
    the addition undoes (stats["wrapped"]), and samples above the nominal 2^bits - 1 passing through (stats["above_nominal"])."""
    prod = ((s - d) * a) & 0xffffffff
    total = (d << bits) + prod
    stats["wrapped"] += int((total >> 32 != 0).sum())
    t = (total & 0xffffffff) >> bits
    t = np.where(t >= 1 << 31, t - (1 << 32), t)
    stats["saturated"] += int(((t < 0) | (t > 65535)).sum())
    out = np.clip(t, 0, 65535)
    stats["above_nominal"] += int((out >= 1 << bits).sum())
    return out


def _blend_planes(fmt, src, sw, sh, xpos, ypos, alpha, dst, dw, dh, mode):
    planes, x_round, y_round = plane_geometry(fmt)
    bits = depth_bits(fmt)
    if mode == SOURCE:
        alpha = 1.0
    if alpha == 0.0:
        return dst
    if x_round:
        xpos = (xpos + 1) & ~1
    if y_round:
        ypos = (ypos + 1) & ~1
    xoff, yoff = max(-xpos, 0), max(-ypos, 0)
    xpos, ypos = max(xpos, 0), max(ypos, 0)
    if xoff >= sw or yoff >= sh:
        return dst
    bw, bh = min(sw - xoff, dw - xpos), min(sh - yoff, dh - ypos)
    if bw <= 0 or bh <= 0:
        return dst
    s_str, s_off = frame_layout(fmt, sw, sh)
    d_str, d_off = frame_layout(fmt, dw, dh)
    rng = (1 << bits) - 1
    a = min(max(int(alpha * rng), 0), rng)
    for i, (ws, hs, pb) in enumerate(planes):
        cw, ch = _up(bw, ws), _up(bh, hs)                           # sizes round up
        cx, cxo = _up(xpos, ws), _up(xoff, ws)                      # x position and offset round up
        cy, cyo = (ypos >> hs, yoff >> hs)                          # y position and offset round down
        sp = _plane_view(src, s_str[i], s_off[i], _up(sh, hs))[cyo:cyo + ch, cxo * pb:(cxo + cw) * pb]
        dp = _plane_view(dst, d_str[i], d_off[i], _up(dh, hs))[cy:cy + ch, cx * pb:(cx + cw) * pb]
        if alpha == 1.0:
            dp[...] = sp
        elif bits == 8:
            dp[...] = _blend_u8(dp.astype(np.int64), sp.astype(np.int64), a).astype(np.uint8)
        else:
            d16, s16 = np.ascontiguousarray(dp).view("<u2").astype(np.int64), np.ascontiguousarray(sp).view("<u2").astype(np.int64)
            dp[...] = _blend_deep(d16, s16, a, bits).astype("<u2").view(np.uint8)
    return dst


def _fill_planes(kind, fmt, dst, dw, dh, c1, c2, c3):
    planes, _x, _y = plane_geometry(fmt)
    bits = depth_bits(fmt)
    base = fmt.split("_")[0]
    strides, offsets = frame_layout(fmt, dw, dh)
    views = [_plane_view(dst, strides[i], offsets[i], _up(dh, hs)) for i, (ws, hs, pb) in enumerate(planes)]
    if base in PACKED_422:                                            # whole macropixels
        y0b, ub, vb = PACKED_422[base]
        n = (dw + 1) // 2
        mp = views[0][:, :4 * n].reshape(dh, n, 4)
        if kind == 0:
            v = _checker_grid(2 * n, np.arange(dh))
            mp[..., y0b], mp[..., y0b + 2], mp[..., ub], mp[..., vb] = v[:, 0::2], v[:, 1::2], 128, 128
        else:
            mp[..., y0b], mp[..., y0b + 2], mp[..., ub], mp[..., vb] = c1, c1, c2, c3
        return dst
    if base in RGB3 or base in XRGB4:
        pb = planes[0][2]
        px = views[0][:, :pb * dw].reshape(dh, dw, pb)
        if kind == 0:                                                 # R, G and B; the x byte stays as it is
            v = _checker_grid(dw, np.arange(dh)).astype(np.uint8)
            for k in (RGB3[base] if base in RGB3 else XRGB4[base][1]):
                px[..., k] = v
        elif base in RGB3:
            for k, c in zip(RGB3[base], (c1, c2, c3)):
                px[..., k] = c
        elif XRGB4[base][0] == 0:                                     # xRGB / xBGR: the colours land in bytes 0, 1 and 3, byte 2 is 0
            first, last = (c1, c3) if base == "xRGB" else (c3, c1)
            px[..., 0], px[..., 1], px[..., 2], px[..., 3] = first, c2, 0, last
        else:
            px[..., XRGB4[base][0]] = 0
            for k, c in zip(XRGB4[base][1], (c1, c2, c3)):
                px[..., k] = c
        return dst
    sb = 2 if bits > 8 else 1
    put = (lambda view, w, val: view[:, :2 * w].view("<u2").__setitem__(Ellipsis, val)) if bits > 8 else (lambda view, w, val: view[:, :w].__setitem__(Ellipsis, val))
    luma = _checker_grid(dw, np.arange(dh)) << (bits - 8) if kind == 0 else c1
    put(views[0], dw, luma)
    cu, cv = ((1 << (bits - 1),) * 2) if kind == 0 else (c2, c3)
    if base in ("NV12", "NV21"):
        cw = _up(dw, 1)
        pair = views[1][:, :2 * cw].reshape(-1, cw, 2)
        pair[..., 0], pair[..., 1] = (cu, cv) if base == "NV12" else (cv, cu)
        return dst
    u_plane, v_plane = (2, 1) if base == "YV12" else (1, 2)
    put(views[u_plane], _up(dw, planes[1][0]), cu)
    put(views[v_plane], _up(dw, planes[1][0]), cv)
    assert sb == planes[0][2]
    return dst


# ---- the two calls of oracle/ref.py ---------------------------------------------------------------------------------------------------------
def compositor_blend(func, fmt, src, sw, sh, xpos, ypos, alpha, dst, dw, dh, y0, y1, mode):
    src = np.ascontiguousarray(src, dtype=np.uint8)
    assert dst.flags["C_CONTIGUOUS"] and dst.dtype == np.uint8
    if fmt in ALPHA_BYTE:
        return _blend_a32(func, fmt, src, sw, sh, xpos, ypos, alpha, dst, dw, dh, y0, y1, mode)
    if fmt in WIDE:
        return _blend_a64(func, fmt, src, sw, sh, xpos, ypos, alpha, dst, dw, dh, y0, y1, mode)
    assert y0 == 0 and y1 >= dh, "the plane formats are blended over all rows"
    return _blend_planes(fmt, src, sw, sh, xpos, ypos, alpha, dst, dw, dh, mode)


def compositor_fill(kind, fn, fmt, dst, dw, dh, y0, y1, c1=0, c2=0, c3=0):
    """kind 0: checker, 1: colour (c1, c2, c3 = R, G, B or Y, U, V)"""
    assert dst.flags["C_CONTIGUOUS"] and dst.dtype == np.uint8
    if fmt in ALPHA_BYTE:
        return _fill_a32(kind, fmt, dst, dw, dh, y0, y1, c1, c2, c3)
    if fmt in WIDE:
        return _fill_a64(kind, fmt, dst, dw, dh, y0, y1, c1, c2, c3)
    assert y0 == 0 and y1 >= dh, "the plane formats are filled over all rows"
    return _fill_planes(kind, fmt, dst, dw, dh, c1, c2, c3)
