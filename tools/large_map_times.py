#!/usr/bin/env python3
"""Step + observe launch on maps larger than 64 x 64 (csrc/mapf_env_large.hip): microseconds per launch from HIP events around K
launches after W warm-up launches, and the fraction of 8 TB/s by algorithmic bytes counted as bench.py's `roofline` counts them
(per environment L*L map cells + 821 bytes per agent of navigation records read and observation written + 1 done byte).
Usage: large_map_times.py [K] [W]   -- prints one markdown table."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mapf_rl_amd as M  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 200
W = int(sys.argv[2]) if len(sys.argv) > 2 else 20
PEAK_GBS = 8000.0
SHAPES = ((4096, 80, 40), (1024, 128, 64))

print("| envs | map | agents | us / launch | algorithmic MB / launch | GB/s | fraction of 8 TB/s |\n|---|---|---|---|---|---|---|")
for E, L, N in SHAPES:
    env = M.VecEnvironment(E, L, N)
    env.reset_envs(None, 0.3, seed=1)
    env.check_status()
    rng = np.random.RandomState(0)
    tape = [torch.from_numpy(rng.randint(0, 5, size=(E, N)).astype(np.int8)).cuda() for _ in range(8)]
    for i in range(W):
        env.step(tape[i % 8])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(K):
        env.step(tape[i % 8])
    t1.record()
    torch.cuda.synchronize()
    env.check_status()
    us = t0.elapsed_time(t1) * 1e3 / K
    alg = E * (L * L + 821 * N + 1)
    gbs = alg / (us * 1e-6) / 1e9
    print("| %d | %dx%d | %d | %.1f | %.1f | %.0f | %.3f |" % (E, L, L, N, us, alg / 1e6, gbs, gbs / PEAK_GBS))
