"""Shared by tests/test_large_map_cpu.py (mapf_generate) and tests/test_large_map_gpu.py (the on-device reset): scenario statistics
at map side 80 against the reference generator's (tests/golden/large_maps.npz (b), made by tests/golden/make_large_goldens.py), with
the statistics and bounds of tests/gen_stats.py: two-sample KS <= 0.05 for density, component count, largest-component share,
start-goal BFS and Manhattan distance; share of agents in the largest component within 0.02."""
from scipy import stats

from tests import gen_stats as GS
from tests import helpers as H


def check(N, L, maps, agents, goals):
    ours = GS.batch_stats(maps, agents, goals)
    z = H.load_npz("large_maps.npz")
    pre = "stat_n%d_l%d_" % (N, L)
    res = {k: float(stats.ks_2samp(z[pre + k], ours[k]).statistic) for k in GS.FIELDS}
    res["in_largest_diff"] = abs(float(z[pre + "in_largest"].mean()) - float(ours["in_largest"].mean()))
    assert ours["dist"].max() < 2147483647, "a goal is unreachable from its start"
    for k in GS.FIELDS:
        assert res[k] <= GS.KS_BOUND, (k, res)
    assert res["in_largest_diff"] <= 0.02, res
    return res
