#!/usr/bin/env python3
"""Same-box A/B of a module-level switch: runs bench.run_job with the switch on / off, interleaved in one process, and prints job times.
    python scripts/ab_bench.py fatezero_amd.video_diffusion.models.attention QKV_FUSION [--rounds R] [--frames 8,16]
--rounds: interleaved on / off rounds that are KEPT per clip length (default 2); one more round runs first and is dropped (caches, clocks).
--frames: clip lengths, each measured in turn in the same process (default 8: the judged 8 f x 512^2 job)."""
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _opt(argv, name, default):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


def main():
    argv = list(sys.argv[1:])
    rounds = int(_opt(argv, "--rounds", 2))
    frames = [int(f) for f in str(_opt(argv, "--frames", "8")).split(",")]
    mod, name = importlib.import_module(argv[0]), argv[1]
    dev = torch.device("cuda:0")
    pipe = bench.build_pipeline(dev)
    for f in frames:
        z0 = torch.randn(1, 4, f, 64, 64, generator=torch.Generator().manual_seed(1234)).to(dev)
        times = {True: [], False: []}
        for rnd in range(rounds + 1):
            for val in (True, False):
                setattr(mod, name, val)
                torch.cuda.synchronize()
                t0 = time.time()
                bench.run_job(pipe, z0, 50, dev)
                torch.cuda.synchronize()
                if rnd > 0:
                    times[val].append(time.time() - t0)
        print(f"{f} frames x 512^2, 50 + 50 DDIM steps, {rounds} rounds kept (first dropped), interleaved on / off")
        for val in (True, False):
            print(f"  {name}={val}: " + " ".join(f"{t:.4f}" for t in times[val]) + f"  s/job (min {min(times[val]):.4f} median {sorted(times[val])[len(times[val]) // 2]:.4f})")
        on, off = sorted(times[True]), sorted(times[False])
        gain = off[len(off) // 2] - on[len(on) // 2]
        print(f"  median gain {1e3 * gain:.1f} ms/job ({100 * gain / off[len(off) // 2]:.2f} %); slowest on-round {max(on):.4f} vs fastest off-round {min(off):.4f}: "
              f"{'every on-round faster than every off-round' if max(on) < min(off) else 'ROUNDS OVERLAP'}")


main()
