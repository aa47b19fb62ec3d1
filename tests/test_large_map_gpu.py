"""Environments on maps of side 65..128 (mapf_create_large, csrc/mapf_env_large.hip): navigation fields, step + observe, masked
observe, partial loads, status bits, on-device reset and staging, and the Python entry points, all against the sequential C oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import mapf_rl_amd

    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return mapf_rl_amd


def _np(t):
    return t.cpu().numpy()


def _seam_scenarios(E, L, N, rho, seed):
    """random_scenarios with a free band around the 64-bit word seam (columns 60..67) and free border rows / columns, and the first
    agents of every environment started on the seam and on the border, so that the tapes below move them across both."""
    rng = np.random.RandomState(seed)
    maps = (rng.random_sample((E, L, L)) < rho).astype(np.int8)
    maps[:, :, 60:68] = 0
    maps[:, [0, L - 1], :] = 0
    maps[:, :, [0, L - 1]] = 0
    agents = np.zeros((E, N, 2), np.int16)
    goals = np.zeros((E, N, 2), np.int16)
    fixed = [(5, 63), (9, 64), (13, 62), (17, 65), (0, 30), (L - 1, 40), (50, 0), (55, L - 1), (0, 0), (L - 1, L - 1)]
    for e in range(E):
        free = np.argwhere(maps[e] == 0)
        taken = set()
        pick = []
        for c in fixed[:N]:
            pick.append(c)
            taken.add(c)
        for i in rng.permutation(len(free)):
            c = (int(free[i][0]), int(free[i][1]))
            if c not in taken:
                pick.append(c)
                taken.add(c)
            if len(pick) == 2 * N:
                break
        pick = np.array(pick, np.int16)
        agents[e], goals[e] = pick[:N], pick[N:]
    return maps, agents, goals


def _seam_tape(T, E, N, seed):
    """mostly sideways moves (columns 63 <-> 64) with up / down runs, so that border rows and columns are pushed against too"""
    rng = np.random.RandomState(seed)
    tape = rng.randint(0, 5, size=(T, E, N)).astype(np.int8)
    side = rng.random_sample((T, E, N)) < 0.5
    tape[side] = np.where(rng.random_sample(side.sum()) < 0.5, 3, 4)
    tape[: T // 4, :, :] = np.where(np.arange(N) % 2 == 0, 3, 4)[None, None, :]  # runs left / right
    tape[T // 4: T // 2, :, :] = np.where(np.arange(N) % 2 == 0, 1, 2)[None, None, :]  # runs up / down to the borders
    tape[0, :, 0] = 4  # agent 0 starts on column 63 (_seam_scenarios): across the seam to 64 at the first step
    return tape


def _serpentine(L):
    """a map whose only corridor winds through every other row: the path from one end to the other is far longer than 2 L"""
    m = np.zeros((L, L), np.int8)
    for r in range(1, L - 1, 2):
        m[r, :] = 1
        m[r, (L - 1) if (r // 2) % 2 == 0 else 0] = 0
    return m


def test_create_large_ranges(M):
    from mapf_rl_amd import _lib
    import ctypes

    h = ctypes.c_void_p()
    assert _lib.lib.mapf_create_large(2, 80, 8, 4, 0, ctypes.byref(h)) == 0 and h.value
    assert _lib.lib.mapf_map_len(h) == 80
    assert _lib.lib.mapf_destroy(h) == 0
    for L in (64, 129):
        h = ctypes.c_void_p()
        assert _lib.lib.mapf_create_large(2, L, 8, 4, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED and not h.value
    with pytest.raises(ValueError):
        M.VecEnvironment(2, 129, 8)


@pytest.mark.parametrize("L", [65, 80, 100, 127, 128])
def test_navi_equals_oracle(M, L):
    E, N = 3, 4
    for rho in (0.1, 0.3, 0.45):
        maps, agents, goals = H.random_scenarios(E, L, N, rho, seed=L * 7 + int(rho * 100))
        if rho == 0.3:
            maps[0] = _serpentine(L)
            goals[0, 0] = (0, 0)
            agents[0, 0] = (L - 1, L - 1) if ((L - 2) // 2) % 2 == 0 else (L - 1, 0)
            free = np.argwhere(maps[0] == 0)
            rest = free[np.random.RandomState(L).permutation(len(free))]
            rest = [c for c in rest if tuple(c) not in {(0, 0), tuple(agents[0, 0])}][: 2 * (N - 1)]
            agents[0, 1:], goals[0, 1:] = np.array(rest[: N - 1]), np.array(rest[N - 1:])
            d = oracle.dist(maps[0], goals[0, 0])
            assert 2 * L < d[agents[0, 0, 0], agents[0, 0, 1]] < 2147483647  # a path longer than 2 L
        env = M.VecEnvironment(E, L, N)
        env.load(maps, agents, goals)
        env.check_status()
        assert np.array_equal(_np(env.navi_map()), oracle.navi_batch(maps, goals)), (L, rho)
        assert np.array_equal(_np(env.maps()), maps)


@pytest.mark.parametrize("E,L,N,rho,T", [
    (8, 80, 16, 0.3, 40),
    (4, 128, 64, 0.3, 32),
    (2, 100, 200, 0.1, 12),   # N > 64: four wavefronts per environment
    (8, 65, 1, 0.2, 40),      # a single agent
    (4, 127, 10, 0.45, 32),
])
def test_differential_vs_oracle_every_step(M, E, L, N, rho, T):
    maps, agents, goals = _seam_scenarios(E, L, N, rho, seed=E * 1000 + L * 10 + N)
    env = M.VecEnvironment(E, L, N)
    env.load(maps, agents, goals)
    nv = oracle.navi_batch(maps, goals)
    assert np.array_equal(_np(env.navi_map()), nv)
    obs, pos = env.observe()
    for e in range(E):
        assert np.array_equal(_np(obs[e]), oracle.observe(maps[e], agents[e], nv[e]))
    tape = _seam_tape(T, E, N, seed=N + L)
    RD = env.obs_bits_row_dwords
    bits = torch.zeros((E, RD), dtype=torch.int32, device="cuda")
    got_pos = np.zeros((T, E, N, 2), np.int16)
    got_rc = np.zeros((T, E, N), np.int8)
    got_done = np.zeros((T, E), np.uint8)
    crossed = np.zeros(E, bool)
    for t in range(T):
        obs, pos, rew, done, rc = env.step(torch.from_numpy(tape[t]).cuda(), obs_bits_out=bits)
        got_pos[t], got_rc[t], got_done[t] = _np(pos), _np(rc), _np(done)
        assert np.array_equal(_np(rew), H.REWARD_VALUES.astype(np.float32)[got_rc[t]])
        o = _np(obs)
        b = np.unpackbits(_np(bits).view(np.uint8), axis=1, bitorder="little")[:, : N * 486].reshape(E, N, 6, 9, 9)
        assert np.array_equal(b, o)
        for e in range(E):
            assert np.array_equal(o[e], oracle.observe(maps[e], got_pos[t, e], nv[e])), (t, e)
        prev = agents if t == 0 else got_pos[t - 1]
        crossed |= ((prev[..., 1] <= 63) != (got_pos[t][..., 1] <= 63)).any(axis=1)
    env.check_status()
    ref = oracle.rollout(maps, agents, goals, nv, tape, want_obs_last=True)
    assert ref["status"] == 0
    assert np.array_equal(got_pos, ref["pos"]) and np.array_equal(got_rc, ref["rclass"]) and np.array_equal(got_done, ref["done"])
    assert np.array_equal(_np(obs), ref["obs_last"])
    assert np.array_equal(_np(env.steps()), np.full(E, T, np.int32))
    assert crossed.all()  # every environment had an agent cross the column 63 / 64 seam
    assert (got_rc == 3).any()  # collisions (the border, obstacles, other agents) happened


def test_masked_observe_partial_load_and_status_bits(M):
    E, L, N = 16, 96, 12
    maps, agents, goals, _ = M.generate_scenarios(E, L, N, 0.2, seed=4)
    env = M.VecEnvironment(E, L, N)
    env.load(maps, agents, goals)
    RD = env.obs_bits_row_dwords
    bits = torch.zeros((E, RD), dtype=torch.int32, device="cuda")
    tape = H.random_tape(3, E, N, seed=1)
    for t in range(3):
        env.step(torch.from_numpy(tape[t]).cuda(), obs_bits_out=bits)
    # mapf_load_envs: only the listed environments change (map, positions, goals, fields, step counter)
    m2, a2, g2, _ = M.generate_scenarios(3, L, N, 0.3, seed=8)
    ids = np.array([1, 7, 12], np.int32)
    before_navi = _np(env.navi_map()).copy()
    env.load_envs(ids, m2, a2, g2)
    env.check_status()
    maps_now, nav_now = _np(env.maps()), _np(env.navi_map())
    maps_exp = maps.copy()
    maps_exp[ids] = m2
    assert np.array_equal(maps_now, maps_exp)
    keep = np.setdiff1d(np.arange(E), ids)
    assert np.array_equal(nav_now[keep], before_navi[keep])
    assert np.array_equal(nav_now[ids], oracle.navi_batch(m2, g2))
    assert np.array_equal(_np(env.agents_pos())[ids], a2) and (_np(env.steps())[ids] == 0).all() and (_np(env.steps())[keep] == 3).all()
    # mapf_observe_masked: exactly the flagged environments are rewritten
    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")
    mask[ids] = 1
    full_obs = torch.empty((E, N, 6, 9, 9), dtype=torch.uint8, device="cuda")
    env.observe(obs_out=full_obs)
    sent = torch.full_like(full_obs, 7)
    sbits = torch.full_like(bits, -1)
    env.observe(obs_out=sent, obs_bits_out=sbits, mask=mask)
    s = _np(sent)
    assert np.array_equal(s[ids], _np(full_obs)[ids]) and (s[keep] == 7).all() and (_np(sbits)[keep] == -1).all()
    # sticky status bits as on small maps: a bad action, an overlap
    acts = torch.zeros((E, N), dtype=torch.int8, device="cuda")
    acts[2, 3] = 5
    env.step(acts)
    with pytest.raises(AssertionError):
        env.check_status()
    env.step(torch.zeros((E, N), dtype=torch.int8, device="cuda"))
    env.check_status()
    a = _np(env.agents_pos()).copy()
    a[0, 1] = a[0, 0]
    env.set_agents(torch.from_numpy(a).cuda())
    env.step(torch.zeros((E, N), dtype=torch.int8, device="cuda"))
    with pytest.raises(RuntimeError):
        env.check_status()


def _check_invariants(maps, agents, goals, L, N):
    assert set(np.unique(maps)) <= {0, 1}
    for e in range(maps.shape[0]):
        cells = np.concatenate([agents[e], goals[e]]).astype(np.int64)
        assert cells.min() >= 0 and cells.max() < L
        assert len(np.unique(cells[:, 0] * L + cells[:, 1])) == 2 * N
        assert maps[e][cells[:, 0], cells[:, 1]].sum() == 0


@pytest.mark.parametrize("E,L,N,rho", [(32, 80, 16, 0.3), (16, 128, 64, -1.0), (16, 100, 1, 0.45)])
def test_reset_invariants_navi_reachability(M, E, L, N, rho):
    env = M.VecEnvironment(E, L, N)
    env.reset_envs(None, rho, seed=11)
    env.check_status()
    maps, agents, goals = _np(env.maps()), _np(env.agents_pos()), _np(env.goals_pos())
    _check_invariants(maps, agents, goals, L, N)
    assert np.array_equal(_np(env.navi_map()), oracle.navi_batch(maps, goals))
    for e in range(E):
        for i in range(min(N, 8)):
            d = oracle.dist(maps[e], goals[e, i])
            assert d[agents[e, i, 0], agents[e, i, 1]] < 2147483647
    if rho > 0:
        assert abs(maps.mean() - rho) < 0.02
    else:
        assert 0.1 < maps.mean() < 0.35  # triangular(0, 0.33, 0.5) has mean 0.277
    # a masked reset touches only the flagged environments
    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")
    mask[1::3] = 1
    env.reset_envs(mask, rho, seed=11)
    env.check_status()
    m2, nav2 = _np(env.maps()), _np(env.navi_map())
    f = _np(mask).astype(bool)
    assert np.array_equal(m2[~f], maps[~f]) and not np.array_equal(m2[f], maps[f])
    assert np.array_equal(nav2, oracle.navi_batch(m2, _np(env.goals_pos())))


@pytest.mark.parametrize("L,N", [(80, 16), (128, 8)])
def test_staged_reset_equals_direct(M, L, N):
    E = 16
    direct, staged = M.VecEnvironment(E, L, N), M.VecEnvironment(E, L, N)
    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")
    mask[::2] = 1
    for env in (direct, staged):
        env.reset_envs(None, -1.0, seed=5)
    staged.stage_next(-1.0, seed=5)
    for rnd in range(3):
        direct.reset_envs(mask, -1.0, seed=5)
        staged.reset_envs(mask, -1.0, seed=5)
        staged.stage_next(-1.0, seed=5)
        for a, b in ((direct.maps(), staged.maps()), (direct.agents_pos(), staged.agents_pos()), (direct.goals_pos(), staged.goals_pos()),
                     (direct.navi_map(), staged.navi_map()), (direct.steps(), staged.steps())):
            assert torch.equal(a, b), rnd
        mask = 1 - mask
    direct.check_status()
    staged.check_status()


def test_multi_handle_set_rejects_large_handles(M):
    from mapf_rl_amd import _lib
    from mapf_rl_amd.environment import MultiEnvironment

    env = M.VecEnvironment(8, 80, 4)
    env.reset_envs(None, 0.2, seed=1)
    with pytest.raises(_lib.MapfError) as ex:
        MultiEnvironment([env], [torch.zeros((8, 4), dtype=torch.int8, device="cuda")], [None], [torch.zeros(8, dtype=torch.uint8, device="cuda")])
    assert ex.value.status == _lib.ERR_UNSUPPORTED


def test_single_env_facade_at_80(M):
    env = M.Environment(map_length=80, num_agents=16)
    assert env.map_size == (80, 80) and env.num_agents == 16
    obs, pos = env.reset()
    assert obs.shape == (16, 6, 9, 9) and obs.dtype == bool and pos.shape == (16, 2) and pos.dtype == np.int64
    assert env.navi_map.shape == (16, 4, 88, 88) and env.navi_map.dtype == bool
    nv = oracle.navi(env.map.astype(np.int8), env.goals_pos.astype(np.int16))
    assert np.array_equal(env.navi_map[:, :, 4:-4, 4:-4], nv.astype(bool))
    rng = np.random.RandomState(0)
    ag = env.agents_pos.astype(np.int16)
    for t in range(6):
        acts = [int(x) for x in rng.randint(0, 5, 16)]
        (obs, pos), rewards, done, info = env.step(acts)
        st, ag, rc, dn = oracle.step(env.map.astype(np.int8), ag, env.goals_pos.astype(np.int16), np.array(acts, np.int8))
        assert st == 0 and np.array_equal(pos, ag) and info == {"step": t} and isinstance(rewards, list) and len(rewards) == 16
        assert np.array_equal(obs, oracle.observe(env.map.astype(np.int8), ag, nv).astype(bool))
    with pytest.raises(AssertionError):
        env.step([5] + [0] * 15)


def test_vectorised_evaluation_equals_sequential_at_80(M):
    from mapf_rl_amd import evaluate as EV
    from mapf_rl_amd.model import Network

    K, L, N, steps_max = 32, 80, 16, 10
    maps, agents, goals, _ = M.generate_scenarios(K, L, N, 0.3, seed=21)
    tests = {"maps": [m.astype(np.float32) for m in maps], "agents": [a.astype(np.int64) for a in agents],
             "goals": [g.astype(np.int64) for g in goals]}
    torch.manual_seed(3)
    net = Network().cuda().eval()
    f_rate, mean_steps, steps, ok = EV.evaluate(net, tests, max_steps=steps_max, num_cases=K)
    for i in range(K):
        env = M.Environment()
        env.load(tests["maps"][i], tests["agents"][i], tests["goals"][i])
        done = False
        net.reset()
        while not done and env.steps < steps_max:
            obs, pos = env.observe()
            actions, _, _, _ = net.step(torch.from_numpy(obs.astype(np.float32)), torch.from_numpy(pos.astype(np.float32)))
            _, _, done, _ = env.step(actions)
        assert env.steps == steps[i]
        assert bool(np.array_equal(env.agents_pos, env.goals_pos)) == bool(ok[i])
    assert 0.0 <= f_rate <= 1.0 and mean_steps <= steps_max


def test_actor_on_device_reset_with_staging_at_80(M):
    from mapf_rl_amd.actor import VecActor
    from mapf_rl_amd.model import Network

    torch.manual_seed(0)
    E, L, N = 8, 80, 8
    maps, agents, goals, _ = M.generate_scenarios(E, L, N, 0.2, seed=5)
    env = M.VecEnvironment(E, L, N)
    env.load(maps, agents, goals)
    actor = VecActor(env, Network().cuda().eval(), None, epsilons=0.5, max_steps=6, seed=3, density=0.2, keep_flushed=True)
    first = {}
    for _ in range(20):
        actor.step()
        for ep in actor.flushed:
            first.setdefault(ep["env"], ep)
        if len(first) == E and len(actor.flushed) >= 2 * E:
            break
    assert len(first) == E
    env.check_status()
    for e, ep in first.items():
        nv = oracle.navi(maps[e], goals[e])
        raw = np.unpackbits(ep["obs"].cpu().numpy().view(np.uint8).reshape(ep["obs"].shape[0], -1), axis=1, bitorder="little")
        obs0 = raw[0, : N * 486].reshape(N, 6, 9, 9)
        assert np.array_equal(obs0, oracle.observe(maps[e], agents[e], nv))
    # the environments now play scenarios drawn on the device: consistent with the oracle as well
    m, a, g = _np(env.maps()), _np(env.agents_pos()), _np(env.goals_pos())
    assert np.array_equal(_np(env.navi_map()), oracle.navi_batch(m, g))


def test_train_entry_point_at_80(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--envs", "64", "--agents", "4", "--map", "80", "--capacity", "256",
           "--learning-starts", "2000", "--batch-size", "16", "--max-updates", "6", "--interval", "2"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "start training" in out.stdout
    assert os.path.exists(str(tmp_path / "models" / "6.pth"))


def _fnv1a_rows(b):
    """FNV-1a 64 of every row of a uint8 [K, n] array (the hash oracle.rollout(..., want_hash=True) computes)"""
    h = np.full(b.shape[0], 1469598103934665603, np.uint64)
    p = np.uint64(1099511628211)
    with np.errstate(over="ignore"):
        for j in range(b.shape[1]):
            h = (h ^ b[:, j].astype(np.uint64)) * p
    return h


def test_golden_trajectories_bit_for_bit(M):
    """tests/golden/large_maps.npz (a): the unmodified reference's trajectories at 80x80 / 16 agents and 128x128 / 8 agents --
    positions, rewards (reward classes), done flags and observation hashes of every step."""
    z = H.load_npz("large_maps.npz")
    for N, L, K in z["traj_shapes"]:
        pre = "traj_n%d_l%d_" % (N, L)
        env = M.VecEnvironment(int(K), int(L), int(N))
        env.load(z[pre + "maps"], z[pre + "agents"], z[pre + "goals"])
        tape = z[pre + "tape"]
        for t in range(tape.shape[0]):
            obs, pos, rew, done, rc = env.step(torch.from_numpy(tape[t]).cuda())
            assert np.array_equal(_np(pos), z[pre + "pos"][t]), (L, t)
            assert H.rewards_match(_np(rc), z[pre + "rewards"][t]), (L, t)
            assert np.array_equal(_np(done), z[pre + "done"][t]), (L, t)
            assert np.array_equal(_fnv1a_rows(_np(obs).reshape(int(K), -1)), z[pre + "obs_hash"][t]), (L, t)
        env.check_status()


@pytest.mark.parametrize("N,E", [(16, 4000), (64, 2000)])
def test_reset_matches_reference_statistics_at_80(M, N, E):
    """the on-device reset (component-weighted placement, rejection of exhausted partitions, triangular density) against the
    reference generator's statistics at 80 x 80 (tests/golden/large_maps.npz (b)): two-sample KS <= 0.05 for density, component
    count, largest-component share, start-goal BFS and Manhattan distance (tests/large_stats.py)."""
    from tests import large_stats as LS

    env = M.VecEnvironment(E, 80, N)
    env.reset_envs(None, -1.0, seed=23)
    env.check_status()
    LS.check(N, 80, _np(env.maps()), _np(env.agents_pos()), _np(env.goals_pos()))


def test_test_py_creates_and_evaluates_an_80_fixture(tmp_path):
    """`python test.py --create 16 80` (through evaluate.create_test, fewer cases) then `python test.py --test-case` on it with a
    checkpoint in --model-dir"""
    from mapf_rl_amd import evaluate as EV
    from mapf_rl_amd.model import Network

    fx = str(tmp_path / "test16_80.pkl")
    EV.create_test(16, 80, test_num=4, seed=1, path=fx, with_opt_steps=True)
    (tmp_path / "models").mkdir()
    torch.manual_seed(0)
    torch.save(Network().state_dict(), str(tmp_path / "models" / "0.pth"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--test-case", fx, "--model-dir", str(tmp_path / "models"), "--start", "0"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "finish:" in out.stdout and "mean steps:" in out.stdout
