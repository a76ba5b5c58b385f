"""GPU: waves as the general host planner now packs them — nb mixed inside a
wave, the lanes filled by the knapsack, read lengths differing inside a wave —
give every pair the oracle's bits. Prepared batches (hcphmm.Batch) take the
host planner; the plan each case relies on is checked first through the
dry-run hooks. Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import packing_cases as P

pytestmark = pytest.mark.gpu


def assert_same(res, ref, what):
    """Bit-exact: raw fp32, rescue flags, raw fp64 of the rescued, log10."""
    assert np.array_equal(res["raw_f32"].view(np.uint32), ref["raw_f32"].view(np.uint32)), what
    assert np.array_equal(res["rescued"], ref["rescued"]), what
    m = ref["rescued"].astype(bool)
    assert np.array_equal(res["raw_f64"][m].view(np.uint64), ref["raw_f64"][m].view(np.uint64)), what
    assert np.array_equal(res["loglik"].view(np.uint64), ref["loglik"].view(np.uint64)), what


def run_batch(engine, b):
    bt = engine.Batch(b)
    try:
        bt.run()
        return bt.results(), bt.stats()
    finally:
        bt.close()


def test_one_bin_mixed_nb_waves(engine, oracle_lib):
    """One width, nb = 2 ... 10 side by side in waves filled to 64 lanes, R
    differing inside a wave."""
    b = P.one_bin()
    with P.columns(50, 0):
        w, wid, R, H, nb, steps = P.wave_table(*P.plan(P.bind(engine.lib()), b))
        res, st = run_batch(engine, b)
    assert set(w[:, 3]) == {50} and set(nb) == set(range(2, 11))
    lanes = np.bincount(wid, weights=nb)
    assert (lanes == 64).sum() >= 60 and (w[:, 1] > w[:, 2]).sum() > len(w) // 2
    assert_same(res, oracle_lib.pairs(b, nthreads=16), "one bin")


def test_wave_closes_at_a_width_change(engine, oracle_lib):
    """300 pairs over the widths on both sides of the step from two lanes per
    pair to three: the last wave of a width closes with lanes free where the
    next width begins."""
    b = P.two_widths()
    with P.columns(64):
        w, wid, R, H, nb, steps = P.wave_table(*P.plan(P.bind(engine.lib()), b))
        res, st = run_batch(engine, b)
    lanes = np.bincount(wid, weights=nb)
    change = np.flatnonzero(w[1:, 3] != w[:-1, 3])
    assert (lanes[change] < 64).sum() >= 2 and {2, 3} <= set(nb)
    assert_same(res, oracle_lib.pairs(b, nthreads=16), "two widths")


def test_in_wave_rescue_in_a_mixed_wave(engine, oracle_lib):
    """One read of all-low qualities among 40 pairs: its fp32 sum underflows
    and the wave that holds it, beside pairs of other nb, rescues it."""
    b = P.low_quality_read()
    ref = oracle_lib.pairs(b, nthreads=16)
    assert ref["rescued"][17] and ref["rescued"].sum() == 1
    with P.columns(50, 0):
        pairs, order, n_seg, waves = P.plan(P.bind(engine.lib()), b)
        res, st = run_batch(engine, b)
    w, wid, R, H, nb, steps = P.wave_table(pairs, order, n_seg, waves)
    mine = wid[np.flatnonzero(order[:n_seg] == 17)[0]]
    assert len(set(nb[wid == mine])) >= 3
    assert_same(res, ref, "low-quality read")
    assert st.n_rescued == 1
