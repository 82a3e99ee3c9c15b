"""Time of gstamd_audio_volume_process_many: stereo buffers at the element's buffer size (1024 frames), one and 64 in a call, and
at 2^22 frames in place and out of place, F32LE and S24LE, and F32LE with per-frame gains.

  python scripts/bench_audio_volume.py          # on an MI355X; prints one JSON line per case

Per case: us per call (device events around ROUNDS calls on one stream after WARMUP calls; the median of REPEATS repeats, the spread (max - min) /
median), the launches of a call, and the achieved bytes/s over the bytes the algorithm needs - the input read once, the output written once, 8
bytes of gains per frame where there are gains - beside the measured copy ceiling of the chip (6.29 TB/s).  The 1024-frame cases stay in
the caches and measure launches: judge them by launches and us per call.  The 2^22-frame cases are judged against the copy ceiling; their buffers
(32 MiB F32LE, 24 MiB S24LE, and as much again out of place) fit the 256 MiB Infinity Cache, which every round finds warm: a share above 1 there
is the cache's doing.  The last case, 2^25 frames out of place (256 MiB read, 256 MiB written), does not fit and is the one that meets HBM.  The fixed
volume is 0.7 (the scaling rows)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS, REPEATS, WARMUP = 2, 5, 10
COPY_CEILING = 6.29e12
BPS = {"F32LE": 4, "S24LE": 3}
# format, buffers, frames, out of place, gains, rounds
CASES = (("F32LE", 1, 1024, False, False, 20000), ("F32LE", 64, 1024, False, False, 20000),
         ("F32LE", 1, 1 << 22, False, False, 5000), ("F32LE", 1, 1 << 22, True, False, 5000),
         ("S24LE", 1, 1 << 22, False, False, 5000), ("S24LE", 1, 1 << 22, True, False, 5000),
         ("F32LE", 1, 1 << 22, False, True, 5000),
         ("F32LE", 1, 1 << 25, True, False, 500))


def algorithmic_bytes(fmt, buffers, frames, gains):
    return buffers * frames * (2 * CHANNELS * BPS[fmt] + (8 if gains else 0))


def main():
    import numpy as np
    import torch
    from gstreamer_amd import audio as A
    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for fmt, buffers, frames, oop, gains, rounds in CASES:
        rng = np.random.RandomState(buffers + frames)
        size = frames * CHANNELS * BPS[fmt]

        def samples():
            if fmt == "F32LE":
                return torch.from_numpy(rng.uniform(-1, 1, frames * CHANNELS).astype(np.float32).view(np.uint8)).to(dev)
            return torch.from_numpy(rng.randint(0, 256, size).astype(np.uint8)).to(dev)

        src = [samples() for _ in range(buffers)]
        dst = [torch.empty(size, dtype=torch.uint8, device=dev) for _ in range(buffers)] if oop else [None] * buffers
        g = torch.from_numpy(np.linspace(1.3, 0.2, frames)).to(dev) if gains else None
        arr = A.volume_buffers([A.volume_buffer(s, d, frames, 0.7, False, g) for s, d in zip(src, dst)])
        for _ in range(WARMUP):
            A.volume_process_many(fmt, CHANNELS, arr, stream)
        torch.cuda.synchronize()
        times = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                A.volume_process_many(fmt, CHANNELS, arr, stream)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / rounds)
        times.sort()
        us = times[len(times) // 2]
        nbytes = algorithmic_bytes(fmt, buffers, frames, gains)
        print(json.dumps(dict(case="%d x %s stereo, %d frames, %s%s" % (buffers, fmt, frames, "out of place" if oop else "in place",
                                                                        ", gains" if gains else ""),
                              us_per_call=round(us, 2), spread=round((times[-1] - times[0]) / us, 3), launches=A.volume_debug()["launches"],
                              algorithmic_bytes=nbytes, achieved_bytes_per_s=round(nbytes / (us * 1e-6), -6), copy_ceiling_bytes_per_s=COPY_CEILING,
                              share_of_copy_ceiling=round(nbytes / (us * 1e-6) / COPY_CEILING, 3))), flush=True)


if __name__ == "__main__":
    main()
