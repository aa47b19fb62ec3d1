#!/usr/bin/env python3
"""Generates tests/golden/large_maps.npz from the UNMODIFIED reference (ZiyuanMa/MAPF_RL) run through oracle/ref_harness.py, for
environments on maps larger than 64 x 64 (the reference's Environment has no cap on map_length).  Build container only; the
output is data.

(a) trajectories: for (N, L) in TRAJ_SHAPES, K scenarios at obstacle density 0.3 (Bernoulli map from a seeded RandomState, starts
    and goals drawn without replacement from the largest free component, map_partition environment.py:21-70), loaded into the
    reference's Environment (load, :198-215, builds get_navi_map :217-276) and stepped T times (:278-430) on a seeded action tape
    (80 % "follow a navigation flag of the own cell", 20 % uniform, tests/golden/make_goldens.py's heuristic):
      traj_n{N}_l{L}_maps     i8  [K][L][L]
      traj_n{N}_l{L}_agents   i16 [K][N][2]       start positions
      traj_n{N}_l{L}_goals    i16 [K][N][2]
      traj_n{N}_l{L}_tape     i8  [T][K][N]       the executed actions
      traj_n{N}_l{L}_pos      i16 [T][K][N][2]    positions after each step
      traj_n{N}_l{L}_rewards  f64 [T][K][N]       the reference's rewards (reward classes map onto them, config.py:8-12)
      traj_n{N}_l{L}_done     u8  [T][K]
      traj_n{N}_l{L}_obs_hash u64 [T][K]          FNV-1a 64 over the step's observation bytes (uint8 [N][6][9][9]), the hash
                                                  oracle.rollout(..., want_hash=True) computes
(b) generator statistics at (N, L) in STAT_SHAPES, S seeded reference constructions each (Environment.__init__, :75-144), in the
    schema of tests/golden/make_gen_stats.py: stat_n{N}_l{L}_{rho, ncomp, largest_frac, dist, manhattan, in_largest, failures}.

Usage:  python tests/golden/make_large_goldens.py
"""
import multiprocessing as mp
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))
TRAJ_SHAPES = [(16, 80, 3), (8, 128, 2)]  # (agents, map side, scenarios)
T = 64
STAT_SHAPES = [(16, 80), (64, 80)]
S = 2000


def fnv1a(b):
    h = 1469598103934665603
    for v in b:
        h = ((h ^ int(v)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def gen_trajectories(ref, data):
    from tests.golden.make_goldens import heuristic_actions

    for N, L, K in TRAJ_SHAPES:
        pre = "traj_n%d_l%d_" % (N, L)
        maps = np.zeros((K, L, L), np.int8)
        agents = np.zeros((K, N, 2), np.int16)
        goals = np.zeros((K, N, 2), np.int16)
        tape = np.zeros((T, K, N), np.int8)
        pos = np.zeros((T, K, N, 2), np.int16)
        rew = np.zeros((T, K, N), np.float64)
        done = np.zeros((T, K), np.uint8)
        hs = np.zeros((T, K), np.uint64)
        for k in range(K):
            rng = np.random.RandomState(1000 * L + 10 * N + k)
            m = (rng.random_sample((L, L)) < 0.3).astype(np.int8)
            parts = ref.environment.map_partition(m)
            big = max(parts, key=len)
            pick = [big[i] for i in rng.permutation(len(big))[: 2 * N]]
            maps[k], agents[k], goals[k] = m, pick[:N], pick[N:]
            env = ref.environment.Environment()
            env.load(m.astype(np.int64), agents[k].astype(np.int64), goals[k].astype(np.int64))
            obs, _ = env.observe()
            for t in range(T):
                acts = heuristic_actions(obs, rng, 0.8)
                (obs, p), r, d, info = env.step([int(x) for x in acts])
                assert info["step"] == t
                tape[t, k], pos[t, k], rew[t, k], done[t, k] = acts, p, r, d
                hs[t, k] = fnv1a(obs.astype(np.uint8).tobytes())
            print(pre, "scenario", k, "done steps", int(done[:, k].sum()), flush=True)
        for name, v in (("maps", maps), ("agents", agents), ("goals", goals), ("tape", tape), ("pos", pos), ("rewards", rew),
                        ("done", done), ("obs_hash", hs)):
            data[pre + name] = v


def _stat_work(args):
    k, (N, L), lo, hi = args
    from oracle import ref_harness as rh
    from tests.golden.make_gen_stats import scenario_stats

    ref = rh.load_reference()
    ref.environment.Environment.get_navi_map = lambda self: None  # statistics of the scenario only (see make_gen_stats.py)
    out, fails = [], 0
    for s in range(lo, hi):
        np.random.seed(200000 * (k + 1) + s)
        random.seed(200000 * (k + 1) + s)
        try:
            env = ref.environment.Environment(num_agents=N, map_length=L)
        except ValueError:
            fails += 1
            continue
        out.append(scenario_stats(np.asarray(env.map), env.agents_pos, env.goals_pos))
    return k, out, fails


def gen_stats(data):
    jobs = [(k, shape, lo, min(S, lo + 50)) for k, shape in enumerate(STAT_SHAPES) for lo in range(0, S, 50)]
    res = {k: ([], 0) for k in range(len(STAT_SHAPES))}
    with mp.Pool(8) as pool:
        for k, out, fails in pool.imap_unordered(_stat_work, jobs):
            res[k] = (res[k][0] + out, res[k][1] + fails)
    data["stat_S"] = np.array(S)
    for k, (N, L) in enumerate(STAT_SHAPES):
        out, fails = res[k]
        pre = "stat_n%d_l%d_" % (N, L)
        data[pre + "rho"] = np.array([o["rho"] for o in out], np.float32)
        data[pre + "ncomp"] = np.array([o["ncomp"] for o in out], np.int16)
        data[pre + "largest_frac"] = np.array([o["largest_frac"] for o in out], np.float32)
        data[pre + "dist"] = np.array([v for o in out for v in o["dist"]], np.int16)
        data[pre + "manhattan"] = np.array([v for o in out for v in o["manhattan"]], np.int16)
        data[pre + "in_largest"] = np.array([v for o in out for v in o["in_largest"]], np.uint8)
        data[pre + "failures"] = np.array(fails, np.int32)
        print(pre, len(out), "scenarios, failures", fails, "rho mean %.4f dist mean %.2f" % (data[pre + "rho"].mean(), data[pre + "dist"].mean()))


def main():
    from oracle import ref_harness as rh

    data = {"traj_shapes": np.array(TRAJ_SHAPES), "stat_shapes": np.array(STAT_SHAPES)}
    gen_stats(data)
    gen_trajectories(rh.load_reference(), data)
    np.savez_compressed(os.path.join(OUT, "large_maps.npz"), **data)
    print("large_maps.npz", len(data), "arrays")


if __name__ == "__main__":
    main()
