"""The `amdaudioconvert` element over the big-endian, unsigned and 20-bit formats (-m gpu): caps with the new formats negotiate on both of
its pads, and what a pipeline writes is what the C ABI's converter gives for the same bytes - and, where the runtime's registry has the stock
CPU `audioconvert` (an independent implementation of the same rules), what that writes for the integer formats without dither.  Runtimes are
found, and their absence skipped, as in tests/test_plugin_gpu.py."""
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
FORMATS = ["S16BE", "U16LE", "S24BE", "S20LE", "F32BE"]
FRAMES, BUFFERS = 1024, 6


@pytest.fixture(scope="module", params=["1.14", "1.29"])
def gst_env(request, native_lib, tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "plugins"))
    import build as plugin_build
    env = dict(os.environ)
    tmp = tmp_path_factory.mktemp("gstaf" + request.param.replace(".", ""))
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
        env["LD_PRELOAD"] = sys_stdcpp
    return env, tmp


def launch(env, pipeline, check=True):
    r = subprocess.run([env["GSTAMD_LAUNCH_BIN"], "-q"] + pipeline.split(), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-3000:]
    return r


def convert_blocks(gpu, ifmt, ofmt, raw, channels=2):
    """the C ABI's converter (dither none) over `raw` in the element's buffers of FRAMES frames"""
    import torch
    cv = A.AudioConverter(A.audio_info(ifmt, 48000, channels), A.audio_info(ofmt, 48000, channels), A.audio_converter_config(dither_method="none"))
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


def caps(fmt):
    return "audio/x-raw,format=%s,rate=48000,channels=2,layout=interleaved" % fmt


@pytest.mark.parametrize("fmt", FORMATS)
def test_element_negotiates_and_converts_the_new_formats(gst_env, gpu, fmt):
    env, tmp = gst_env
    fin, fmid, fback = tmp / ("af_in_%s.s16" % fmt), tmp / ("af_mid_%s.raw" % fmt), tmp / ("af_back_%s.s32" % fmt)
    src = np.random.RandomState(A.AFMT[fmt]).randint(0, 256, FRAMES * BUFFERS * 4).astype(np.uint8)
    src.tofile(fin)
    # the new format on the source pad ...
    launch(env, "filesrc location=%s blocksize=%d ! %s ! amdaudioconvert dithering=none ! %s ! filesink location=%s" % (fin, FRAMES * 4, caps("S16LE"), caps(fmt), fmid))
    mid = np.fromfile(fmid, np.uint8)
    exp = convert_blocks(gpu, "S16LE", fmt, src)
    assert mid.shape == exp.shape and (mid == exp).all(), (fmt, mid.shape, exp.shape)
    # ... and on the sink pad
    launch(env, "filesrc location=%s blocksize=%d ! %s ! amdaudioconvert dithering=none ! %s ! filesink location=%s"
           % (fmid, FRAMES * 2 * A.AFMT_BYTES[fmt], caps(fmt), caps("S32LE"), fback))
    back = np.fromfile(fback, np.uint8)
    exp = convert_blocks(gpu, fmt, "S32LE", mid)
    assert back.shape == exp.shape and (back == exp).all(), (fmt, back.shape, exp.shape)
    if fmt[0] == "F":
        return
    # the stock CPU element, where this runtime has it
    fcpu, fcpu_back = tmp / ("af_cpu_%s.raw" % fmt), tmp / ("af_cpu_back_%s.s32" % fmt)
    r = launch(env, "filesrc location=%s blocksize=%d ! %s ! audioconvert dithering=none ! %s ! filesink location=%s" % (fin, FRAMES * 4, caps("S16LE"), caps(fmt), fcpu),
               check=False)
    if r.returncode != 0:
        assert "audioconvert" in r.stdout, r.stdout[-2000:]     # no such element in this runtime: nothing to compare with
        return
    cpu = np.fromfile(fcpu, np.uint8)
    assert cpu.shape == mid.shape and (cpu == mid).all(), (fmt, "stock audioconvert", int((cpu != mid).sum()))
    launch(env, "filesrc location=%s blocksize=%d ! %s ! audioconvert dithering=none ! %s ! filesink location=%s"
           % (fmid, FRAMES * 2 * A.AFMT_BYTES[fmt], caps(fmt), caps("S32LE"), fcpu_back))
    cpu = np.fromfile(fcpu_back, np.uint8)
    assert cpu.shape == back.shape and (cpu == back).all(), (fmt, "stock audioconvert back", int((cpu != back).sum()))
