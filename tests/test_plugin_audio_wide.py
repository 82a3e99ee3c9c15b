"""The `amdaudioconvert` element with more than 8 channels (-m gpu): caps of up to 64 channels negotiate, and what a pipeline writes is what the C
ABI's wide converter (gstamd_audio_converter_new_wide) gives for the same buffers - unpositioned 12-channel frames, a 16 -> 2
`mix-matrix`, 12 channels from frames to planes.  A stereo pipeline still makes its converter with gstamd_audio_converter_new_layouts (the element's
debug line says which constructor it called).  Runtimes are found, and their absence skipped, as in tests/test_plugin_audio_layouts.py."""
import numpy as np
import pytest

from gstreamer_amd import audio as A
from test_plugin_audio_layouts import gst_env, launch, FRAMES, BUFFERS      # noqa: F401 (gst_env is a fixture)

pytestmark = pytest.mark.gpu


def caps(fmt, channels, planar=False, mask=0):
    return "audio/x-raw,format=%s,rate=48000,channels=%d,channel-mask=(bitmask)0x%x,layout=%s" % (fmt, channels, mask, "non-interleaved" if planar else "interleaved")


def convert_blocks(gpu, ifmt, ofmt, in_ch, out_ch, raw, ol=0, dither="tpdf", matrix=None):
    """ONE wide converter of the C ABI over `raw` in the element's buffers of FRAMES frames"""
    import torch
    cv = A.AudioConverterWide(A.audio_info_wide(ifmt, 48000, in_ch, None, unpositioned=in_ch > 2),
                              A.audio_info_wide(ofmt, 48000, out_ch, None, unpositioned=out_ch > 2),
                              A.audio_converter_config(dither_method=dither), in_layout=0, out_layout=ol, mix_matrix=matrix)
    ibpf, obpf = A.AFMT_BYTES[ifmt] * in_ch, A.AFMT_BYTES[ofmt] * out_ch
    out = []
    for off in range(0, raw.size, FRAMES * ibpf):
        blk = raw[off: off + FRAMES * ibpf]
        n = blk.size // ibpf
        d_in = torch.from_numpy(blk.copy()).to(gpu)
        d_out = torch.zeros(n * obpf, dtype=torch.uint8, device=gpu)
        cv.samples(d_in, n, d_out, n)
        torch.cuda.synchronize()
        out.append(d_out.cpu().numpy())
    cv.free()
    return np.concatenate(out)


def run(env, tmp, tag, src, in_caps, props, out_caps, block):
    fin, fout = tmp / ("aw_%s.in" % tag), tmp / ("aw_%s.out" % tag)
    src.tofile(fin)
    r = launch(env, "filesrc location=%s blocksize=%d ! %s ! amdaudioconvert %s ! %s ! filesink location=%s" % (fin, block, in_caps, props, out_caps, fout))
    return np.fromfile(fout, np.uint8), r.stdout


def debug_env(env):
    e = dict(env)
    e.update(GST_DEBUG="amdaudioconvert:5", GST_DEBUG_NO_COLOR="1")
    return e


def test_twelve_unpositioned_channels(gst_env, gpu):
    env, tmp = gst_env
    src = np.random.RandomState(12).randint(0, 256, FRAMES * BUFFERS * 12 * 2).astype(np.uint8)
    got, log = run(debug_env(env), tmp, "12", src, caps("S16LE", 12), "", caps("F32LE", 12), FRAMES * 2 * 12)
    exp = convert_blocks(gpu, "S16LE", "F32LE", 12, 12, src)
    assert got.shape == exp.shape and (got == exp).all()
    assert "through gstamd_audio_converter_new_wide" in log and "through gstamd_audio_converter_new_layouts" not in log


def test_sixteen_to_stereo_with_a_mix_matrix(gst_env, gpu):
    env, tmp = gst_env
    rng = np.random.RandomState(16)
    matrix = [[float(np.float32(v)) for v in row] for row in rng.uniform(-0.3, 0.3, (2, 16))]
    prop = "mix-matrix=<" + ",".join("<" + ",".join("(float)%r" % v for v in row) + ">" for row in matrix) + ">"
    src = rng.uniform(-1.1, 1.1, FRAMES * BUFFERS * 16).astype(np.float32).view(np.uint8)
    got, _ = run(env, tmp, "16", src, caps("F32LE", 16), prop, caps("S16LE", 2, mask=3), FRAMES * 4 * 16)
    exp = convert_blocks(gpu, "F32LE", "S16LE", 16, 2, src, matrix=matrix)            # tpdf is the element's default
    assert got.shape == exp.shape and (got == exp).all()


def test_twelve_channels_from_frames_to_planes(gst_env, gpu):
    env, tmp = gst_env
    src = np.random.RandomState(7).uniform(-1.1, 1.1, FRAMES * BUFFERS * 12).astype(np.float32).view(np.uint8)
    got, _ = run(env, tmp, "12p", src, caps("F32LE", 12), "", caps("S16LE", 12, planar=True), FRAMES * 4 * 12)
    exp = convert_blocks(gpu, "F32LE", "S16LE", 12, 12, src, ol=1)
    assert got.shape == exp.shape and (got == exp).all()


def test_stereo_still_goes_through_the_old_constructor(gst_env, gpu):
    env, tmp = gst_env
    src = np.random.RandomState(2).uniform(-1.1, 1.1, FRAMES * BUFFERS * 2).astype(np.float32).view(np.uint8)
    got, log = run(debug_env(env), tmp, "2", src, caps("F32LE", 2, mask=3), "", caps("S16LE", 2, mask=3), FRAMES * 4 * 2)
    assert got.size == FRAMES * BUFFERS * 2 * 2
    assert "through gstamd_audio_converter_new_layouts" in log and "through gstamd_audio_converter_new_wide" not in log
