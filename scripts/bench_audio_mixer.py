"""Time of gstamd_audio_mixer_mix: 16 and 64 stereo F32 inputs summed into one buffer, at the element's buffer size (1024 frames) and at
2^20 frames.

  python scripts/bench_audio_mixer.py           # on an MI355X; prints one JSON line per case

Per case: us per call (device events around ROUNDS calls on one stream after WARMUP calls; the median of REPEATS repeats, the spread (max - min) /
median), the launches of a call, and the achieved bytes/s over the bytes the algorithm needs - every input read once, the output written once -
beside the measured copy ceiling of the chip (6.29 TB/s).  The 1024-frame cases stay in the caches and measure launches: judge them by
launches per call.  The 2^20-frame cases are judged against the copy ceiling; the 16-input one (134 MB of inputs) fits the 256 MiB Infinity Cache,
the 64-input one (537 MB) does not.  Half of the inputs have volume 1.0 (the plain add), half 0.5 (the scaled one)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS, BPS, REPEATS, WARMUP = 2, 4, 5, 10
COPY_CEILING = 6.29e12
CASES = ((16, 1024, 500), (64, 1024, 500), (16, 1 << 20, 50), (64, 1 << 20, 20))    # inputs, frames, rounds


def algorithmic_bytes(n_inputs, frames):
    return (n_inputs + 1) * frames * CHANNELS * BPS


def main():
    import numpy as np
    import torch
    from gstreamer_amd import audio as A
    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for n_inputs, frames, rounds in CASES:
        rng = np.random.RandomState(n_inputs + frames)
        src = [torch.from_numpy(rng.uniform(-1, 1, frames * CHANNELS).astype(np.float32)).to(dev) for _ in range(n_inputs)]
        out = torch.empty(frames * CHANNELS, dtype=torch.float32, device=dev)
        arr = A.mixer_inputs([A.mixer_input(t, 0, frames, 1.0 if k % 2 else 0.5) for k, t in enumerate(src)])
        for _ in range(WARMUP):
            A.mixer_mix("F32LE", CHANNELS, arr, out, frames, stream)
        torch.cuda.synchronize()
        times = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                A.mixer_mix("F32LE", CHANNELS, arr, out, frames, stream)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / rounds)
        times.sort()
        us = times[len(times) // 2]
        nbytes = algorithmic_bytes(n_inputs, frames)
        print(json.dumps(dict(case="%d x F32LE stereo, %d frames" % (n_inputs, frames), us_per_call=round(us, 2),
                              spread=round((times[-1] - times[0]) / us, 3), launches=A.mixer_debug()["launches"], algorithmic_bytes=nbytes,
                              achieved_bytes_per_s=round(nbytes / (us * 1e-6), -6), copy_ceiling_bytes_per_s=COPY_CEILING,
                              share_of_copy_ceiling=round(nbytes / (us * 1e-6) / COPY_CEILING, 3))), flush=True)


if __name__ == "__main__":
    main()
