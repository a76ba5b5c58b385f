"""CPU: how the general host planner packs column-segmented waves (planner.cpp
plan_general: sort_seg_pairs, then pack_seg_waves over seg_pack.hpp
pack_segment; HC_PHMM_TRACE phases "seg sort" and "seg pack: fill"; the packing
alone runs under the sanitizers in test_seg_pack_host.py). Pairs are sorted by (BC, steps =
R + nb - 1) descending; the first unused pair opens a wave and fixes its step
count, and a knapsack over the 64-entry look-ahead fills the other lanes. The
plans are read through the dry-run hooks as test_planner.py does. Lane
efficiency = useful cells / sum(64 * BC * nsteps); the bounds on S2 lie
between the parent's plans (0.9261 / 0.9077) and the packing's model (0.9515 /
0.9360), the others are the parent's own figures, which must not get worse."""
import numpy as np
import pytest

import hcphmm
import packing_cases as P
import workloads as W


@pytest.fixture(scope="module")
def L():
    return P.bind(hcphmm.lib())


@pytest.fixture(scope="module")
def plans(L):
    """Each batch planned once: name -> (batch R, batch H, plan)."""
    cases = {
        "S2-20k": W.config("S2", 20_000),
        "S2-3k": W.config("S2", 3_000),
        "S1": W.config("S1"),
        "S4": W.config("S4"),
        "uniform": W.generate(5_000, (250, 250), (101, 101), 0.01, seed=3),
    }
    out = {k: (b["R"].astype(np.int64), b["H"].astype(np.int64), P.plan(L, b)) for k, b in cases.items()}
    b = P.one_bin()
    with P.columns(50, 0):
        out["one-bin"] = (b["R"].astype(np.int64), b["H"].astype(np.int64), P.plan(L, b))
    return out


@pytest.fixture(scope="module")
def s2_last_part(L):
    """S2 at 1M pairs: hcx_plan_pairs cuts it into 8 parts, the dump is the last."""
    return P.plan(L, W.config("S2"))


def check_plan(pairs, order, n_seg, waves, R, H):
    """What phmm_seg_kernel needs of a plan (test_planner.py check_plan,
    re-stated): every pair in one slot, the waves partitioning the slots,
    each wave's pairs on at most 64 lanes of its width, its row bounds and
    step count covering them."""
    n = len(R)
    assert len(pairs) == n
    assert np.array_equal(pairs[:, 1], R) and np.array_equal(pairs[:, 3], H)
    assert len(np.unique(order)) == len(order) == n
    assert n_seg == n
    w, wid, Rs, Hs, nb, steps = P.wave_table(pairs, order, n_seg, waves)
    starts = np.concatenate([[0], np.cumsum(w[:, 4])[:-1]])
    assert np.array_equal(w[:, 0], starts) and w[:, 4].sum() == n_seg
    assert set(w[:, 3]) <= P.WIDTHS and w[:, 4].min() >= 1 and w[:, 4].max() <= 64
    nw = len(w)
    assert np.bincount(wid, weights=nb, minlength=nw).max() <= 64
    first = starts
    assert np.array_equal(w[:, 1], np.maximum.reduceat(Rs, first))
    assert np.array_equal(w[:, 2], np.minimum.reduceat(Rs, first))
    assert np.array_equal(w[:, 5], np.maximum.reduceat(steps, first))
    return w, wid, nb, steps


@pytest.mark.parametrize("name", ["S2-20k", "S2-3k", "uniform", "one-bin"])
def test_plan_invariants(plans, name):
    R, H, pl = plans[name]
    check_plan(*pl, R, H)


def test_one_bin_is_one_width_with_mixed_waves(plans):
    """The hand-made batch is what it is meant to be: one width, nb = 2 ... 10,
    and waves that hold several nb side by side with R differing inside."""
    R, H, pl = plans["one-bin"]
    w, wid, nb, steps = check_plan(*pl, R, H)
    assert set(w[:, 3]) == {50}
    assert set(nb) == set(range(2, 11))
    assert not any(64 % c == 0 for c in np.bincount(nb)[2:])
    kinds = np.array([len(set(nb[wid == k])) for k in range(len(w))])
    assert (kinds >= 3).sum() > len(w) // 2
    assert (w[:, 1] > w[:, 2]).sum() > len(w) // 2
    # 4 193 lanes in all: 65 full waves and a rest, if nothing is lost; the
    # last waves of the list have few pairs left to choose from
    lanes = np.bincount(wid, weights=nb)
    assert nb.sum() == 4193 and len(w) <= 67 and (lanes == 64).sum() >= 60


@pytest.mark.parametrize("name,eff_min,empty_max", [
    ("S2-20k", 0.930, 0.005),
    ("S2-3k", 0.650, None),
    ("S1", 0.761, None),
    ("S4", 0.696, None),
])
def test_lane_efficiency(plans, name, eff_min, empty_max):
    eff, empty = P.lane_stats(*plans[name][2])
    print(f"{name}: lane efficiency {eff:.4f}, empty-lane share {empty:.4f}, {len(plans[name][2][3])} waves")
    assert eff >= eff_min
    if empty_max is not None:
        assert empty <= empty_max


def test_lane_efficiency_s2_1m_last_part(s2_last_part):
    eff, empty = P.lane_stats(*s2_last_part)
    print(f"S2 1M last part: lane efficiency {eff:.4f}, empty-lane share {empty:.4f}, {len(s2_last_part[3])} waves")
    assert eff >= 0.948
    assert empty <= 0.004


@pytest.mark.parametrize("name", ["S2-20k", "S2-3k", "S1", "S4", "uniform", "one-bin"])
def test_first_pair_sets_the_step_count(plans, name):
    """A wave runs as long as the pair that opened it: no later pair of the
    sorted list lengthens it."""
    pairs, order, n_seg, waves = plans[name][2]
    w, wid, R, H, nb, steps = P.wave_table(pairs, order, n_seg, waves)
    assert np.array_equal(w[:, 5], steps[w[:, 0]])


def test_first_pair_sets_the_step_count_s2_1m(s2_last_part):
    pairs, order, n_seg, waves = s2_last_part
    w, wid, R, H, nb, steps = P.wave_table(pairs, order, n_seg, waves)
    assert np.array_equal(w[:, 5], steps[w[:, 0]])


@pytest.mark.parametrize("name", ["S2-20k", "one-bin"])
def test_planning_is_deterministic(L, plans, name):
    if name == "S2-20k":
        again = P.plan(L, W.config("S2", 20_000))
    else:
        with P.columns(50, 0):
            again = P.plan(L, P.one_bin())
    for x, y in zip(plans[name][2], again):
        assert np.array_equal(x, y)
