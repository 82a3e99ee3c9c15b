"""Time per call of the resampler in INTERPOLATED filter mode: k_fir_interp_lds / k_fir_interp_lds_many against the library of the
parent commit, where such a stream is k_fir + k_history and resample_many sends interpolated streams one by one.

  python scripts/bench_audio_interp.py [--parent-lib PATH/libgstamddsp.so]    # prints one JSON line per setting and library run

1024-frame stereo F32 buffers, 48000 -> 44101 (filter mode auto picks the interpolated table, 8x oversampled), three settings: cubic, one stream
(gstamd_audio_resampler_resample); linear, one stream; cubic, 64 streams through one gstamd_audio_resampler_resample_many.  Every library run is a
process of its own - one process loads one library - and with --parent-lib the two alternate: parent, this tree, parent, this tree.  Times are device
events around ROUNDS calls on one stream after WARMUP calls; each figure is the median of REPEATS repeats, `spread` is (max - min) / median of those
repeats.  The last line compares: per setting the two runs of each library, the parent's own run-to-run difference, and this / parent.  The buffers
stay in the caches: this measures launches and the kernels' latency, not HBM."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, REPEATS, WARMUP = 1024, 7, 200
SETTINGS = (("cubic_1", "cubic", 1, 4000), ("linear_1", "linear", 1, 4000), ("cubic_64_many", "cubic", 64, 400))


def measure(label):
    import numpy as np
    import torch
    from gstreamer_amd import audio as A
    dev = torch.device("cuda")
    have_record = hasattr(A.lib(), "gstamd_audio_resampler_debug_launches")
    for name, kind, streams, rounds in SETTINGS:
        opts = A.options("kaiser", 4, 48000, 44101, filter_interpolation=kind)
        rs = [A.AudioResampler("F32LE", 2, 48000, 44101, "kaiser", opts) for _ in range(streams)]
        assert rs[0].debug()["filter_mode"] == A.FILTER_MODE["interpolated"]
        rng = np.random.RandomState(1)
        src = [torch.from_numpy(rng.uniform(-1, 1, FRAMES * 2).astype(np.float32)).to(dev) for _ in range(streams)]
        dst = [torch.zeros((FRAMES + 16) * 2, dtype=torch.float32, device=dev) for _ in range(streams)]   # the output length moves by a frame from buffer to buffer
        sp, dp = [t.data_ptr() for t in src], [t.data_ptr() for t in dst]

        def one():
            rs[0].resample(sp[0], FRAMES, dp[0], rs[0].get_out_frames(FRAMES))

        def many():
            A.resample_many(rs, sp, [FRAMES] * streams, dp, [r.get_out_frames(FRAMES) for r in rs])

        fn = one if streams == 1 else many
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
        row = dict(library=label, setting=name, streams=streams, frames=FRAMES, rounds=rounds, call_us=round(times[len(times) // 2], 2),
                   spread=round((times[-1] - times[0]) / times[len(times) // 2], 3))
        if have_record:
            row["record"] = A.resample_debug()
        for r in rs:
            r.free()
        print(json.dumps(row), flush=True)


def main():
    if "--worker" in sys.argv:
        measure(sys.argv[sys.argv.index("--worker") + 1])
        return
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    rows = []
    for label, lib in ([("parent", parent), ("this", None)] * 2 if parent else [("this", None)]):
        env = dict(os.environ)
        env.setdefault("HIP_FORCE_DEV_KERNARG", "1")            # as the tests and bench.py run (gstreamer_amd/csrc/tuning.cpp)
        env.pop("GSTAMD_LIB_PATH", None)
        if lib:
            env["GSTAMD_LIB_PATH"] = os.path.abspath(lib)
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--worker", label], env=env, text=True)
        sys.stdout.write(out)
        sys.stdout.flush()
        rows += [json.loads(line) for line in out.splitlines() if line.startswith("{")]
    if parent:
        summary = {}
        for name, _, _, _ in SETTINGS:
            p = [r["call_us"] for r in rows if r["setting"] == name and r["library"] == "parent"]
            t = [r["call_us"] for r in rows if r["setting"] == name and r["library"] == "this"]
            summary[name] = dict(parent_us=p, this_us=t, parent_run_to_run=round(abs(p[0] - p[1]) / min(p), 3),
                                 this_over_parent=round((sum(t) / len(t)) / (sum(p) / len(p)), 3))
        print(json.dumps(dict(summary=summary)), flush=True)


if __name__ == "__main__":
    main()
