"""Child process of test_video_strip_interior.py: GSTAMD_FAST_VARIANT is read once per process, so every value of it needs a process of its own.

python strip_variant_child.py CASE.npz  - converts the case's frames on the GPU as one list and one by one, under the variant the environment
names, and compares both with the expected bytes in the file.  Prints one line per mismatch and exits 1, else exits 0.  No torch here: frames
go through the library's own device-memory helpers, which keeps the start of the process short."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gstreamer_amd import video as V  # noqa: E402


def main(path):
    z = np.load(path)
    ifmt, ofmt, site = str(z["ifmt"]), str(z["ofmt"]), str(z["site"])
    w, h = int(z["w"]), int(z["h"])
    srcs, exp = z["srcs"], z["exp"]
    n = len(srcs)
    L = V.lib()
    ii, oi = V.video_info(ifmt, w, h, chroma_site=site), V.video_info(ofmt, w, h)
    conv = V.VideoConverter(ii, oi)

    def dev(nbytes, host=None):
        p = L.gstamd_device_alloc(nbytes)
        assert p
        host = np.zeros(nbytes, np.uint8) if host is None else np.ascontiguousarray(host)
        assert L.gstamd_device_upload(p, host.ctypes.data, nbytes, None) == 0
        return p

    d_src = [dev(int(ii.size), s) for s in srcs]
    d_lst = [dev(int(oi.size)) for _ in range(n)]
    d_one = [dev(int(oi.size)) for _ in range(n)]
    conv.frames(d_src, d_lst)
    for s, d in zip(d_src, d_one):
        conv.frame(s, d)
    assert L.gstamd_stream_synchronize(None) == 0
    bad = 0
    for name, bufs in (("list", d_lst), ("single", d_one)):
        for i, p in enumerate(bufs):
            got = np.empty(int(oi.size), np.uint8)
            assert L.gstamd_device_download(got.ctypes.data, p, got.size, None) == 0
            diff = int((got != exp[i]).sum())
            if diff:
                bad += 1
                print("%s frame %d: %d bytes differ, first at %d" % (name, i, diff, int(np.flatnonzero(got != exp[i])[0])))
    conv.free()
    for p in d_src + d_lst + d_one:
        L.gstamd_device_free(p)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
