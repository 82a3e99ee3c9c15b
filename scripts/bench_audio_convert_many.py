"""Time of one round of 64 audio conversions, one by one and through gstamd_audio_converter_samples_many:

  python scripts/bench_audio_convert_many.py [--layouts] [--parent-lib PATH/libgstamddsp.so]    # prints one JSON line per case and library

--layouts: the cases of DESIGN 3.8.5 (non-interleaved sides, the wide converter) instead of those of 3.8.4.

A round is one buffer for each of 64 stereo converters of one plan.  Per plan it is timed as 64 gstamd_audio_converter_samples calls ("loop")
and as one gstamd_audio_converter_samples_many call ("many"); with --parent-lib the loop is also timed on that library (a build of the commit
before the batched entry), in a process of its own - one process loads one library - and the two libraries alternate.  Times are device events
around ROUNDS rounds on one stream after WARMUP rounds; each figure is the median of REPEATS repeats, the spread (max - min) / median.  The
buffers of the small cases stay in the caches: they measure launches, not HBM.  The last case (64 x 48000 frames) moves 35 MB a round."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, REPEATS, ROUNDS, WARMUP = 64, 5, 200, 20
CASES = (("F32LE->S16LE tpdf", 1024, 48000, dict(dither_method="tpdf")),
         ("F32LE->S16LE tpdf high", 1024, 48000, dict(dither_method="tpdf", noise_shaping="high")),
         ("F32LE 48000->S16LE 44100 tpdf kaiser", 1024, 44100, dict(dither_method="tpdf", resampler_method="kaiser")),
         ("F32LE->S16LE tpdf", 48000, 48000, dict(dither_method="tpdf")))
# (name, frames, out_rate, config, in_layout, out_layout, (in_ch, out_ch) of a wide converter or None)
LAYOUT_CASES = (("F32LE planar->S16LE tpdf", 1024, 48000, dict(dither_method="tpdf"), 1, 0, None),
                ("F32LE planar->S16LE planar tpdf high", 1024, 48000, dict(dither_method="tpdf", noise_shaping="high"), 1, 1, None),
                ("F32LE planar 48000->S16LE planar 44100 tpdf kaiser", 1024, 44100, dict(dither_method="tpdf", resampler_method="kaiser"), 1, 1, None),
                ("wide F32LE 16ch->S16LE 6ch planar tpdf", 1024, 48000, dict(dither_method="tpdf"), 0, 1, (16, 6)),
                ("F32LE planar->S16LE tpdf", 48000, 48000, dict(dither_method="tpdf"), 1, 0, None))


def measure(label, layouts=False):
    import numpy as np
    import torch
    from gstreamer_amd import audio as A
    dev = torch.device("cuda")
    have_many = hasattr(A._conv_lib(), "gstamd_audio_converter_samples_many")
    for name, frames, out_rate, cfg, il, ol, wide in (LAYOUT_CASES if layouts else [c + (0, 0, None) for c in CASES]):
        rounds = ROUNDS if frames <= 1024 else 50
        in_ch, out_ch = wide or (2, 2)
        if wide:                                # a dense matrix, the same for all: one run
            m = np.random.RandomState(2).uniform(-1, 1, (out_ch, in_ch)) / in_ch
            cvs = [A.AudioConverterWide(A.audio_info_wide("F32LE", 48000, in_ch), A.audio_info_wide("S16LE", out_rate, out_ch), A.audio_converter_config(**cfg),
                                        in_layout=il, out_layout=ol, mix_matrix=m.tolist()) for _ in range(STREAMS)]
        elif il or ol:
            cvs = [A.AudioConverter(A.audio_info("F32LE", 48000, 2), A.audio_info("S16LE", out_rate, 2), A.audio_converter_config(**cfg), in_layout=il, out_layout=ol)
                   for _ in range(STREAMS)]
        else:
            cvs = [A.AudioConverter(A.audio_info("F32LE", 48000, 2), A.audio_info("S16LE", out_rate, 2), A.audio_converter_config(**cfg)) for _ in range(STREAMS)]
        rng = np.random.RandomState(1)
        src = [torch.from_numpy(rng.uniform(-1, 1, frames * in_ch).astype(np.float32)).to(dev) for _ in range(STREAMS)]
        # a resampler's output length moves by a frame from buffer to buffer: room for the longest, the frames asked for each round
        dst = [torch.zeros((frames + 16) * out_ch, dtype=torch.int16, device=dev) for _ in range(STREAMS)]
        sp, dp = [t.data_ptr() for t in src], [t.data_ptr() for t in dst]

        def loop():
            for c, s, d in zip(cvs, sp, dp):
                c.samples(s, frames, d, c.get_out_frames(frames))

        def many():
            A.convert_many(cvs, sp, [frames] * STREAMS, dp, [c.get_out_frames(frames) for c in cvs])

        row = dict(library=label, case=name, streams=STREAMS, frames=frames, rounds=rounds)
        for mode, fn in (("loop", loop), ("many", many)):
            if mode == "many" and not have_many:
                continue
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(REPEATS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(rounds):
                    fn()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / rounds)
            times.sort()
            row[mode + "_us"], row[mode + "_spread"] = round(times[len(times) // 2], 2), round((times[-1] - times[0]) / times[len(times) // 2], 3)
            if mode == "many":
                row["counters"] = A.convert_many_debug()
        for c in cvs:
            c.free()
        print(json.dumps(row), flush=True)


def main():
    if "--worker" in sys.argv:
        measure(sys.argv[sys.argv.index("--worker") + 1], "--layouts" in sys.argv)
        return
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    # every measurement in a fresh process; with a parent library: parent, this tree, parent, this tree
    for label, lib in ([("parent", parent), ("this", None)] * 2 if parent else [("this", None)]):
        env = dict(os.environ)
        env.pop("GSTAMD_LIB_PATH", None)
        if lib:
            env["GSTAMD_LIB_PATH"] = os.path.abspath(lib)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker", label] + (["--layouts"] if "--layouts" in sys.argv else []), env=env)


if __name__ == "__main__":
    main()
