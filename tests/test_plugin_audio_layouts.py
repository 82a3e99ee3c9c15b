"""The `amdaudioconvert` element with non-interleaved caps (-m gpu): both layouts negotiate on both of its pads, what a pipeline writes is what the
C ABI's converter (gstamd_audio_converter_new_layouts) gives for the same buffers - with the element's default tpdf dither too, which a
non-interleaved output draws plane after plane -, and a non-interleaved stream runs from it into `amdaudioresample` and back.  A buffer that
filesrc cuts from a file carries no GstAudioMeta: its planes are back to back, [channels][frames], which is also how the element writes a
non-interleaved output buffer.  Runtimes are found, and their absence skipped, as in tests/test_plugin_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gstreamer_amd import audio as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GST = "/opt/conda/bin/gst-launch-1.0"
RT129 = os.path.join(ROOT, "oracle", "_ref", "rt129")
LAUNCH129 = os.path.join(ROOT, "plugins", "tests", "launch129")
FRAMES, BUFFERS = 1024, 6
SURROUND = ["front-left", "front-right", "front-center", "lfe1", "rear-left", "rear-right"]


@pytest.fixture(scope="module", params=["1.14", "1.29"])
def gst_env(request, native_lib, tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "plugins"))
    import build as plugin_build
    env = dict(os.environ)
    tmp = tmp_path_factory.mktemp("gstal" + request.param.replace(".", ""))
    if request.param == "1.29":
        so = plugin_build.build129()
        if not so or not os.path.exists(LAUNCH129) or not os.path.exists(os.path.join(RT129, "lib", "libgstvideo-1.0.so.0")):
            pytest.skip("the 1.29 runtime is not built (oracle/rt129_build.py needs /root/reference)")
        plugs = [os.path.join(RT129, "plugins", f) for f in ("libgstcoreelements.so", "libgstvideotestsrc.so", "libgstaudiotestsrc.so")] + [so]
        env.update(GSTAMD_LAUNCH_PLUGINS=":".join(plugs), GSTAMD_RUNTIME="1.29", GSTAMD_LAUNCH_BIN=LAUNCH129,
                   LD_LIBRARY_PATH=os.path.join(RT129, "lib") + ":" + os.path.join(ROOT, "gstreamer_amd", "lib") + ":" + env.get("LD_LIBRARY_PATH", ""))
        return env, tmp
    if not os.path.exists(GST):
        pytest.skip("no GStreamer runtime in this image")
    so = plugin_build.build()
    assert os.path.exists(so)
    env.update(GST_PLUGIN_PATH=os.path.join(ROOT, "plugins") + ":/opt/conda/lib/gstreamer-1.0", GST_PLUGIN_SYSTEM_PATH="/nonexistent",
               GST_REGISTRY=str(tmp / "registry.bin"), GST_REGISTRY_FORK="no", GSTAMD_RUNTIME="1.14", GSTAMD_LAUNCH_BIN=GST,
               LD_LIBRARY_PATH=os.path.join(ROOT, "gstreamer_amd", "lib") + ":" + env.get("LD_LIBRARY_PATH", ""))
    sys_stdcpp = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"      # the conda runtime ships an older libstdc++ than the one hipcc links against
    if os.path.exists(sys_stdcpp):
        env["LD_PRELOAD"] = " ".join(v for v in (sys_stdcpp, env.get("LD_PRELOAD", "")) if v)
    return env, tmp


def launch(env, pipeline):
    r = subprocess.run([env["GSTAMD_LAUNCH_BIN"], "-q"] + pipeline.split(), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return r


def caps(fmt, channels, planar, rate=48000):
    mask = ",channel-mask=(bitmask)0x3f" if channels == 6 else ""
    return "audio/x-raw,format=%s,rate=%d,channels=%d%s,layout=%s" % (fmt, rate, channels, mask, "non-interleaved" if planar else "interleaved")


def convert_blocks(gpu, ifmt, ofmt, il, ol, raw, channels, dither):
    """ONE converter of the C ABI over `raw` in the element's buffers of FRAMES frames, a non-interleaved side as [channels][frames] per buffer"""
    import torch
    pos = SURROUND if channels == 6 else None
    cv = A.AudioConverter(A.audio_info(ifmt, 48000, channels, pos), A.audio_info(ofmt, 48000, channels, pos), A.audio_converter_config(dither_method=dither),
                          in_layout=il, out_layout=ol)
    ibpf, obpf = A.AFMT_BYTES[ifmt] * channels, A.AFMT_BYTES[ofmt] * channels
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


@pytest.mark.parametrize("channels", [2, 6])
@pytest.mark.parametrize("dither", ["none", "tpdf"])
def test_element_converts_between_the_layouts(gst_env, gpu, channels, dither):
    env, tmp = gst_env
    prop = "dithering=none" if dither == "none" else ""         # tpdf is the element's default
    tag = "%d_%s" % (channels, dither)
    rng = np.random.RandomState(channels)
    # non-interleaved F32LE -> interleaved S16LE
    fin, fout = tmp / ("al_in_%s.f32" % tag), tmp / ("al_out_%s.s16" % tag)
    src = rng.uniform(-1.1, 1.1, FRAMES * BUFFERS * channels).astype(np.float32).view(np.uint8)
    src.tofile(fin)
    launch(env, "filesrc location=%s blocksize=%d ! %s ! amdaudioconvert %s ! %s ! filesink location=%s"
           % (fin, FRAMES * 4 * channels, caps("F32LE", channels, True), prop, caps("S16LE", channels, False), fout))
    got = np.fromfile(fout, np.uint8)
    exp = convert_blocks(gpu, "F32LE", "S16LE", 1, 0, src, channels, dither)
    assert got.shape == exp.shape and (got == exp).all(), ("F32LE planes -> S16LE frames", channels, dither, got.shape, exp.shape)
    # interleaved S16LE -> non-interleaved F32LE, and (with a quantizer) -> non-interleaved S8
    for ofmt in ("F32LE", "S8"):
        fback = tmp / ("al_back_%s_%s.raw" % (tag, ofmt))
        launch(env, "filesrc location=%s blocksize=%d ! %s ! amdaudioconvert %s ! %s ! filesink location=%s"
               % (fout, FRAMES * 2 * channels, caps("S16LE", channels, False), prop, caps(ofmt, channels, True), fback))
        back = np.fromfile(fback, np.uint8)
        exp2 = convert_blocks(gpu, "S16LE", ofmt, 0, 1, got, channels, dither)
        assert back.shape == exp2.shape and (back == exp2).all(), ("S16LE frames ->", ofmt, "planes", channels, dither, back.shape, exp2.shape)


def test_element_prefers_the_layout_of_its_input(gst_env, gpu):
    """the peer leaves the layout open: the planes stay planes (S16LE -> S32LE between two non-interleaved sides)"""
    env, tmp = gst_env
    fin, fout = tmp / "al_pref.s16", tmp / "al_pref.s32"
    src = np.random.RandomState(5).randint(0, 256, FRAMES * BUFFERS * 4).astype(np.uint8)
    src.tofile(fin)
    launch(env, "filesrc location=%s blocksize=%d ! %s ! amdaudioconvert ! audio/x-raw,format=S32LE ! filesink location=%s"
           % (fin, FRAMES * 4, caps("S16LE", 2, True), fout))
    got = np.fromfile(fout, np.uint8)
    exp = convert_blocks(gpu, "S16LE", "S32LE", 1, 1, src, 2, "tpdf")
    assert got.shape == exp.shape and (got == exp).all()


def test_planes_run_from_the_converter_into_the_resampler(gst_env):
    """amdaudioconvert ! amdaudioresample with non-interleaved caps between them and back to frames: the samples of the same chain with interleaved caps"""
    env, tmp = gst_env
    fin = tmp / "al_chain.s16"
    np.random.RandomState(9).randint(0, 256, FRAMES * BUFFERS * 4).astype(np.uint8).tofile(fin)
    outs = []
    for planar in (False, True):
        fout = tmp / ("al_chain_%d.s16" % planar)
        launch(env, "filesrc location=%s blocksize=%d ! %s ! amdaudioconvert ! %s ! amdaudioresample ! %s ! amdaudioconvert dithering=none ! %s ! filesink location=%s"
               % (fin, FRAMES * 4, caps("S16LE", 2, False), caps("F32LE", 2, planar), caps("F32LE", 2, planar, 44100), caps("S16LE", 2, False, 44100), fout))
        outs.append(np.fromfile(fout, np.uint8))
    assert outs[0].size > FRAMES * BUFFERS * 4 * 0.85 and outs[0].shape == outs[1].shape and (outs[0] == outs[1]).all()
