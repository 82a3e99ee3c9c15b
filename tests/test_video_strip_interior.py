"""k_convert_strip's straight-line path for interior strips (video_fast.h fast_strip_interior) next to fast_strip, byte for byte (-m gpu).

A wave takes the straight-line path when all its line pairs have both lines and it is not the row's last 256-pixel column; every other wave of
the same launch runs fast_strip.  The sizes put the seam between the two everywhere it can lie:
  widths   256 (one column, which is also the last: fast_strip alone), 260 (a full column plus a one-lane column), 1032 (four full columns plus
           a two-lane column);
  heights  2 and 4 (edge strips only), 14 (8 pairs: at K = 3 a first, one interior and a last strip), 46 (24 pairs);
  frames per frames() call  1 and 2 (store policy 1), 9 (policy 3) - and every frame alone through frame(); the library's own K is 2 for these
           plans, K = 3 and 4 run through GSTAMD_FAST_VARIANT in both block orders (with K = 3 the 14-line frame has one interior strip).
The expected bytes come from the reference where it is built, else from the host emulator (tests/emu, which runs fast_strip for every strip).
Sources are random bytes, so no two lines of a frame and no two frames are alike: a pair stored to the wrong line, a skipped peeled pair or a
frame of a list written to another's buffer fails.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from gstreamer_amd import video as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

WIDTHS = (256, 260, 1032)
HEIGHTS = (2, 4, 14, 46)
COUNTS = (1, 2, 9)
# chroma mode -> (chroma site of the source, converter config): h-cosited sites take CHROMA_H_H2_CS, the others CHROMA_H_H2; chroma-mode=none
# switches the upsampling off (the planner then serves the conversion with its general kernel - the bytes are held to the same oracle)
CHROMA = {"h2cs": ("mpeg2", {}), "h2": ("jpeg", {}), "none": ("mpeg2", dict(chroma_mode="none"))}


@pytest.fixture(scope="module")
def expected(emu_lib):
    """expected(ifmt, ofmt, w, h, site, cfg, src) -> the destination frame's bytes"""
    from oracle import ref
    use_ref = ref.available()
    if use_ref:
        try:
            ref.lib()
        except OSError:
            use_ref = False
    emu_lib.emu_video_convert.argtypes = [C.POINTER(V.VideoInfo), C.POINTER(V.VideoInfo), C.POINTER(V.ConverterConfig), C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_char_p, C.c_int]

    def run(ifmt, ofmt, w, h, site, cfg, src):
        if use_ref:
            return ref.VideoConverter(ifmt, w, h, ofmt, w, h, in_chroma_site=site, config=cases.ref_config_string(ref, cfg)).frame(src)
        ii, oi = V.video_info(ifmt, w, h, chroma_site=site), V.video_info(ofmt, w, h)
        dst = np.zeros(int(oi.size), np.uint8)
        desc = C.create_string_buffer(256)
        r = emu_lib.emu_video_convert(C.byref(ii), C.byref(oi), C.byref(V.converter_config(**cfg)), src.ctypes.data, dst.ctypes.data, 1, desc, 256)
        assert r == 0, desc.value
        return dst
    return run


def sources(ifmt, w, h, n, seed):
    size = int(V.video_info(ifmt, w, h).size)
    return [cases.frame_bytes(size, "random", seed * 131 + i) for i in range(n)]


@pytest.mark.parametrize("chroma", sorted(CHROMA))
@pytest.mark.parametrize("ofmt", ["BGRA", "RGBA", "ARGB", "ABGR"])
@pytest.mark.parametrize("ifmt", ["NV12", "NV21"])
def test_strip_paths_match_the_oracle_bytewise(native_lib, gpu, expected, ifmt, ofmt, chroma):
    import torch
    site, cfg = CHROMA[chroma]
    bad = []
    for w in WIDTHS:
        for h in HEIGHTS:
            ii, oi = V.video_info(ifmt, w, h, chroma_site=site), V.video_info(ofmt, w, h)
            srcs_np = sources(ifmt, w, h, max(COUNTS), w * 64 + h)
            exp = [expected(ifmt, ofmt, w, h, site, cfg, s) for s in srcs_np]
            srcs = [torch.from_numpy(s).to(gpu) for s in srcs_np]
            conv = V.VideoConverter(ii, oi, V.converter_config(**cfg))
            runs = []
            for n in COUNTS:                    # a list of n frames in one frames() call
                outs = [torch.zeros(int(oi.size), dtype=torch.uint8, device=gpu) for _ in range(n)]
                conv.frames(srcs[:n], outs)
                runs.append(("list%d" % n, outs))
            ones = [torch.zeros(int(oi.size), dtype=torch.uint8, device=gpu) for _ in srcs]
            for s, d in zip(srcs, ones):       # the same frames one by one
                conv.frame(s, d)
            runs.append(("single", ones))
            torch.cuda.synchronize()
            for name, outs in runs:
                for i, o in enumerate(outs):
                    got = o.cpu().numpy()
                    if got.size != exp[i].size or not (got == exp[i]).all():
                        bad.append((w, h, name, i, int((got != exp[i]).sum()) if got.size == exp[i].size else -1))
            conv.free()
    assert not bad, bad[:8]


def test_strip_paths_with_the_memory_pipeline_busy(native_lib, gpu, expected):
    """1280 x 720, 9 frames as one list (policy 3) and one by one (policy 1), the library's own K: thousands of waves at once.  A store whose data
    registers the next instruction overwrites too early loses single pixels only when the memory pipeline is backed up - the small frames
    above never show it (video_fast.h store16_buffer)."""
    import torch
    ifmt, ofmt, w, h, n = "NV12", "BGRA", 1280, 720, 9
    ii, oi = V.video_info(ifmt, w, h), V.video_info(ofmt, w, h)
    srcs_np = sources(ifmt, w, h, n, 1280)
    exp = [expected(ifmt, ofmt, w, h, None, {}, s) for s in srcs_np]
    srcs = [torch.from_numpy(s).to(gpu) for s in srcs_np]
    conv = V.VideoConverter(ii, oi)
    bad = []
    for rep in range(3):
        lst = [torch.zeros(int(oi.size), dtype=torch.uint8, device=gpu) for _ in range(n)]
        one = [torch.zeros(int(oi.size), dtype=torch.uint8, device=gpu) for _ in range(n)]
        conv.frames(srcs, lst)
        for s, d in zip(srcs, one):
            conv.frame(s, d)
        torch.cuda.synchronize()
        for name, outs in (("list", lst), ("single", one)):
            for i, o in enumerate(outs):
                diff = int((o.cpu().numpy() != exp[i]).sum())
                if diff:
                    bad.append((rep, name, i, diff))
    conv.free()
    assert not bad, bad[:8]


def run_child(tmp_path, expected, ifmt, ofmt, w, h, n, seed, variant):
    srcs = sources(ifmt, w, h, n, seed)
    exp = [expected(ifmt, ofmt, w, h, "mpeg2", {}, s) for s in srcs]
    case = str(tmp_path / "case.npz")
    np.savez(case, ifmt=ifmt, ofmt=ofmt, site="mpeg2", w=w, h=h, srcs=np.stack(srcs), exp=np.stack(exp))
    env = dict(os.environ, GSTAMD_FAST_VARIANT=variant)
    r = subprocess.run([sys.executable, os.path.join(HERE, "strip_variant_child.py"), case], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]


def test_three_pairs_with_the_memory_pipeline_busy(native_lib, gpu, expected, tmp_path):
    """the same under K = 3 (a loop of two rounds ahead of the peeled pair), 1280 x 720, 9 frames as a list (policy 3) and one by one (policy 1)"""
    run_child(tmp_path, expected, "NV12", "BGRA", 1280, 720, 9, 1283, "0,0,3,0")


@pytest.mark.parametrize("order", [1, 0], ids=["xcd", "grid"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_strip_paths_per_k_and_block_order(native_lib, gpu, expected, tmp_path, K, order):
    """k_convert_strip_xcd (GSTAMD_FAST_VARIANT=0,0,K,1) makes the same choice per wave from its own block map; 0,0,K,0 is k_convert_strip with a
    K the library would not choose itself: lists of 9 frames (policy 3) and single frames (policy 1) of 1032 x 46, K = 2 / 3 / 4 pairs per wave.
    The variant is read once per process, so the conversion runs in a child process."""
    run_child(tmp_path, expected, "NV12", "BGRA", 1032, 46, 9, 7000 + K, "0,0,%d,%d" % (K, order))
