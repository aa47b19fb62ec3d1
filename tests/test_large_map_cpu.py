"""CPU: the constructor of environments on maps of side 65..128 (mapf_create_large, include/mapf_env.h) -- declared, exported,
bound, argument checks before any HIP call -- and the C oracle at those sizes."""
import ctypes
import os
import re

import numpy as np

from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_large_is_declared_exported_and_bound():
    from mapf_rl_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mapf_env.h")).read(), flags=re.S)
    assert re.search(r"\bint mapf_create_large\s*\(int num_envs, int map_len, int num_agents, int obs_radius, int device, mapf_env_t \*\*out\)", src)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mapf_create_large")
    assert "mapf_create_large" in {s[0] for s in _lib.SYMBOLS}


def test_create_large_argument_checks():
    from mapf_rl_amd import _lib

    lib = _lib.lib
    h = ctypes.c_void_p()
    assert lib.mapf_create_large(1, 80, 2, 4, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.mapf_create_large(0, 80, 2, 4, 0, ctypes.byref(h)) == _lib.ERR_INVALID_ARG
    assert lib.mapf_create_large(1, 80, 0, 4, 0, ctypes.byref(h)) == _lib.ERR_INVALID_ARG
    assert lib.mapf_create_large(1, 80, 2, 4, -1, ctypes.byref(h)) == _lib.ERR_INVALID_ARG
    assert lib.mapf_create_large(1, 64, 2, 4, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED   # mapf_create's range
    assert lib.mapf_create_large(1, 10, 2, 4, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert lib.mapf_create_large(1, 129, 2, 4, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert lib.mapf_create_large(1, 80, 256, 4, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert lib.mapf_create_large(1, 80, 2, 3, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert not h.value
    # the small-map constructor keeps its contract
    assert lib.mapf_create(1, 65, 2, 4, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert lib.mapf_abi_version() == 2


def test_create_large_without_device():
    from mapf_rl_amd import _lib

    lib = _lib.lib
    if lib.mapf_device_count() != 0:
        return
    h = ctypes.c_void_p()
    for L in (65, 80, 128):
        assert lib.mapf_create_large(1, L, 2, 4, 0, ctypes.byref(h)) == _lib.ERR_HIP
        assert not h.value


def test_golden_trajectories_reproduced_by_the_oracle():
    """tests/golden/large_maps.npz (a): the unmodified reference stepped on 80x80 / 16-agent and 128x128 / 8-agent scenarios.  The
    C oracle the GPU tests compare against reproduces every step's positions, rewards, done flags and observation hashes."""
    from tests import helpers as H

    z = H.load_npz("large_maps.npz")
    for N, L, K in z["traj_shapes"]:
        pre = "traj_n%d_l%d_" % (N, L)
        maps, agents, goals = z[pre + "maps"], z[pre + "agents"], z[pre + "goals"]
        assert maps.shape == (K, L, L) and agents.shape == (K, N, 2)
        r = oracle.rollout(maps, agents, goals, oracle.navi_batch(maps, goals), z[pre + "tape"], want_hash=True)
        assert r["status"] == 0
        assert np.array_equal(r["pos"], z[pre + "pos"])
        assert H.rewards_match(r["rclass"], z[pre + "rewards"])
        assert np.array_equal(r["done"], z[pre + "done"])
        assert np.array_equal(r["obs_hash"], z[pre + "obs_hash"])


def test_host_generator_matches_reference_statistics_at_80():
    """mapf_generate (the host generator behind generate_scenarios) at (16, 80) and (64, 80) against the reference generator's
    statistics (tests/golden/large_maps.npz (b)): two-sample KS <= 0.05 per statistic, as tests/gen_stats.py does at <= 40."""
    import mapf_rl_amd as M
    from tests import large_stats as LS

    for N, L, E in ((16, 80, 4000), (64, 80, 2000)):
        maps, agents, goals, _ = M.generate_scenarios(E, L, N, -1.0, seed=41)
        LS.check(N, L, maps, agents, goals)


def test_create_test_plans_past_the_reference_horizon_at_80(tmp_path):
    """`test.py --create 16 80`: case 36 of the draw (seed 1) has no plan within the reference's 256-step horizon; on maps larger
    than 64 x 64 the expert plans over L * L steps (evaluate.create_test)."""
    import pickle

    from mapf_rl_amd import evaluate as EV

    path = str(tmp_path / "t16_80.pkl")
    EV.create_test(16, 80, test_num=37, seed=1, path=path, with_opt_steps=True)
    with open(path, "rb") as f:
        d = pickle.load(f)
    assert len(d["maps"]) == 37 and len(d["opt_steps"]) == 37 and d["maps"][0].shape == (80, 80)
    for m, a, g, steps in zip(d["maps"], d["agents"], d["goals"], d["opt_steps"]):
        far = max(int(oracle.dist(np.asarray(m).astype(np.int8), (int(q[0]), int(q[1])))[int(p[0]), int(p[1])]) for p, q in zip(a, g))
        assert steps >= far  # the makespan is at least the longest shortest path
