"""Per-call time of the wide audio converter (gstamd_audio_converter_new_wide):

  python scripts/bench_audio_wide.py            # prints one JSON line per case

1. the wide path against the old one on the same conversion of at most 8 channels (F32LE 6 -> 2, S16LE -> S8 8 -> 8 with tpdf);
2. F32LE 64 -> 2 and 64 -> 64 with a dense matrix: time per call, bytes moved (input + output) over that time, and the bytes the
   per-output-channel form of the old mixer would read (out_ch x the input).
Each figure is the median over REPEATS repeats of the mean of CALLS back-to-back calls on one stream, after WARMUP calls; the spread is
(max - min) / median of the repeats."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gstreamer_amd import audio as A  # noqa: E402

REPEATS, CALLS, WARMUP = 5, 200, 50
L51 = ["front-left", "front-right", "front-center", "lfe1", "rear-left", "rear-right"]


def per_call(cv, d_in, frames, d_out):
    for _ in range(WARMUP):
        cv.samples(d_in, frames, d_out, frames)
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            cv.samples(d_in, frames, d_out, frames)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / CALLS * 1e6)
    times.sort()
    return times[len(times) // 2], (times[-1] - times[0]) / times[len(times) // 2]


def case(name, ifmt, ofmt, in_ch, out_ch, frames, in_pos=None, matrix=None, paths=("old", "wide"), **cfg):
    dev = torch.device("cuda")
    ib, ob = A.AFMT_BYTES[ifmt] * in_ch, A.AFMT_BYTES[ofmt] * out_ch
    rng = np.random.RandomState(1)
    src = rng.uniform(-1, 1, frames * in_ch).astype(np.float32).view(np.uint8) if ifmt[0] == "F" else rng.randint(0, 256, frames * ib).astype(np.uint8)
    d_in, d_out = torch.from_numpy(src).to(dev), torch.zeros(frames * ob, dtype=torch.uint8, device=dev)
    row = dict(case=name, frames=frames, bytes_moved=frames * (ib + ob), old_form_read_bytes=frames * ib * out_ch)
    for path in paths:
        if path == "old":
            cv = A.AudioConverter(A.audio_info(ifmt, 48000, in_ch, in_pos), A.audio_info(ofmt, 48000, out_ch), A.audio_converter_config(mix_matrix=matrix, **cfg))
        else:
            cv = A.AudioConverterWide(A.audio_info_wide(ifmt, 48000, in_ch, in_pos), A.audio_info_wide(ofmt, 48000, out_ch), A.audio_converter_config(**cfg),
                                      mix_matrix=matrix)
        us, spread = per_call(cv, d_in, frames, d_out)
        cv.free()
        row[path + "_us"], row[path + "_spread"] = round(us, 2), round(spread, 3)
        row[path + "_GBps"] = round(row["bytes_moved"] / us / 1e3, 2)
    print(json.dumps(row), flush=True)


def main():
    for frames in (1024, 48000):
        case("F32LE 6->2 (5.1 default matrix)", "F32LE", "F32LE", 6, 2, frames, in_pos=L51)
        case("S16LE->S8 8->8 tpdf", "S16LE", "S8", 8, 8, frames, dither_method="tpdf")
        for out_ch in (2, 64):
            m = (np.random.RandomState(out_ch).uniform(0.1, 1.0, (out_ch, 64)) / 64).astype(np.float32)
            case("F32LE 64->%d dense" % out_ch, "F32LE", "F32LE", 64, out_ch, frames, matrix=[[float(v) for v in r] for r in m], paths=("wide",))


if __name__ == "__main__":
    main()
