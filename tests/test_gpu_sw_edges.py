"""GPU: the HIP Smith-Waterman aligner on the case families of sw_cases.py,
bit for bit against the oracle and the reference's golden outputs: offsets,
CIGAR strings and scores are integers, so there is no tolerance anywhere.
What each family exercises is asserted on the CPU (test_sw_census.py).

layout    batch maxima that size the LDS differently, at 1, 2 and 4 waves per
          workgroup and with the generic DP variant; a pair's answer does not
          depend on the batch it is in.
scores    Batch.results(scores=True) against the oracle's end-point score;
          0 for shortcut pairs; each score at its caller index.
gaps      interior gaps of up to 500 bases from a scanned end point.
boundary  parameter rows on both sides of the fast variant's proof; which
          variant ran comes from the library (hcx_sw_dp_variant), not from the
          test's restatement alone.
order     small batches after a large one in the borrowed workspace.

HC_SW_WPG is read by the library at every launch, but nothing it returns says
how many waves a workgroup had, so these tests cannot tell a library that
ignores the variable from one that honours it. Run on an MI355X: pytest -m gpu.
"""
import ctypes as C

import numpy as np
import pytest

import sw_cases as K
import sw_census as Z
import sw_workloads as S

pytestmark = pytest.mark.gpu

LAYOUT_PARAMS = (S.NEW_SW_PARAMETERS, S.ORIGINAL_DEFAULT)


@pytest.fixture(scope="module")
def sw():
    import hcsw
    hcsw.init(0)
    return hcsw


@pytest.fixture(scope="module")
def golden():
    return K.load_golden()["cases"]


def tag(p):
    return "_".join(map(str, p))


def run_batch(sw, b, params, strategy, shortcut=True):
    bt = sw.Batch(b, params, strategy, shortcut)
    try:
        bt.run()
        return bt.results(scores=True)
    finally:
        bt.close()


def differing(got, want):
    """Indices at which (offsets, cigars[, scores]) differ, with the first three."""
    n = len(want[1])
    assert all(len(x) == n for x in got) and all(len(x) == n for x in want)
    bad = [k for k in range(n) if any(g[k] != w[k] for g, w in zip(got, want))]
    return len(bad), [(k, [g[k] for g in got], [w[k] for w in want]) for k in bad[:3]]


def dp_variant(sw, params, strategy, n1max, n2max):
    f = sw.lib().hcx_sw_dp_variant
    f.argtypes = [sw.Params, C.c_int32, C.c_int32, C.c_int32]
    f.restype = C.c_int
    return f(sw.Params(*params), strategy, n1max, n2max)


# ---- layout and scores ----------------------------------------------------
@pytest.fixture(scope="module")
def layout_expected(sw_oracle_lib, golden):
    """(params, strategy, shortcut) -> (offsets, cigars, scores) of the union
    batch from the oracle; with the shortcut on they are also the golden's."""
    union, where = K.layout_union()
    exp = {}
    for p in LAYOUT_PARAMS:
        for st in S.STRATEGIES:
            for sc in (False, True):
                off, cig = sw_oracle_lib.batch(union, p, st, shortcut=sc, nthreads=8)
                exp[p, st, sc] = (off, cig, sw_oracle_lib.scores(union, p, st, shortcut=sc))
            g_off, g_cig = golden[f"layout_{tag(p)}_{st}"]
            assert np.array_equal(exp[p, st, True][0], g_off) and exp[p, st, True][1] == g_cig
    return union, where, exp


@pytest.mark.parametrize("shape", ["wpg1", "wpg2", "wpg4", "generic"])
def test_layout_batches_every_workgroup_shape(sw, layout_expected, shape, monkeypatch):
    if shape == "generic":          # the default workgroup shape, the cutoff + compare variant
        monkeypatch.setenv("HC_SW_GENERIC", "1")
    else:
        monkeypatch.setenv("HC_SW_WPG", shape[3:])
    union, where, exp = layout_expected
    batches = K.layout_batches()
    ran = 0
    for (p, st, sc), (e_off, e_cig, e_sc) in exp.items():
        assert dp_variant(sw, p, st, 1023, 1024) == (0 if shape == "generic" else 1)
        # every pair inside the tall-and-wide batch ...
        n_bad, first = differing(run_batch(sw, union, p, st, sc), (e_off, e_cig, e_sc))
        assert not n_bad, ("union", p, st, sc, n_bad, first)
        # ... and inside the batch whose maxima size the LDS for it alone
        for name, b in batches:
            ks = where[name]
            want = (e_off[ks], [e_cig[k] for k in ks], e_sc[ks])
            n_bad, first = differing(run_batch(sw, b, p, st, sc), want)
            assert not n_bad, (name, p, st, sc, n_bad, first)
            ran += 1
    assert ran == len(batches) * len(LAYOUT_PARAMS) * len(S.STRATEGIES) * 2


def test_layout_scores_cover_dp_and_shortcut_pairs(layout_expected):
    """The expected side of the layout scores: DP pairs with non-zero scores
    and shortcut pairs (score 0, shortcut on only) both occur."""
    union, _, exp = layout_expected
    mask = S.shortcut_mask(union)
    assert 0 < mask.sum() < len(mask)
    for (p, st, sc), (_, _, e_sc) in exp.items():
        if sc:
            assert not e_sc[mask].any()
        assert np.count_nonzero(e_sc[~mask]) >= len(mask) // 2


def test_scores_land_at_the_caller_index(sw, sw_oracle_lib):
    """Host-shortcut pairs (longer than the aligner's limit, answered before
    the device sees them), device-shortcut pairs and DP pairs interleaved: the
    device's pair d is the caller's pair dev_ids[d] != d."""
    rng = np.random.default_rng(17)
    long1 = S.ACGT[rng.integers(0, 4, 2000)].tobytes()
    long2 = bytearray(S.ACGT[rng.integers(0, 4, 1500)].tobytes())
    long2b = bytes(long2)
    long2[7] ^= 6
    long2[1400] ^= 6
    same = S.ACGT[rng.integers(0, 4, 100)].tobytes()
    dp = [K._gap_pair(rng, 30 + 10 * k, 20, 50, k % 2 == 0) for k in range(5)]
    pairs = [(long1, long1), dp[0], (same, same), dp[1], (long2b, bytes(long2)), (long1[:1600], long1[:1600]),
             dp[2], (same[:64], same[:64]), dp[3], dp[4]]
    b = S.from_pairs(pairs)
    host = [0, 4, 5]
    want = sw_oracle_lib.batch(b, nthreads=8) + (sw_oracle_lib.scores(b),)
    is_dp = ~S.shortcut_mask(b)
    assert list(np.nonzero(is_dp)[0]) == [1, 3, 6, 8, 9] and len(set(want[2][is_dp])) == 5 and want[2][is_dp].all()
    assert not want[2][~is_dp].any()
    bt = sw.Batch(b)
    bt.run()
    assert bt.stats()["n_shortcut"] == len(host) + 2
    got = bt.results(scores=True)
    bt.close()
    n_bad, first = differing(got, want)
    assert not n_bad, (n_bad, first)


# ---- long gaps ------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in K.gap_pairs()])
def test_long_gaps_every_strategy_and_param_set(sw, sw_oracle_lib, golden, name):
    b = dict(K.gap_pairs())[name]
    for p in S.PARAM_SETS:
        for st in S.STRATEGIES:
            got = run_batch(sw, b, p, st)
            g_off, g_cig = golden[f"{name}_{tag(p)}_{st}"]
            n_bad, first = differing(got[:2], (g_off, g_cig))
            assert not n_bad, ("golden", name, p, st, n_bad, first)
            n_bad, first = differing(got[:2], sw_oracle_lib.batch(b, p, st, nthreads=8))
            assert not n_bad, ("oracle", name, p, st, n_bad, first)
            e_sc = sw_oracle_lib.scores(b, p, st)
            assert np.array_equal(got[2], e_sc), (name, p, st, np.nonzero(got[2] != e_sc)[0][:5])
            # the same through the borrowed workspace
            flat = sw.align_flat(b, p, st)
            n_bad, first = differing(flat, (g_off, g_cig))
            assert not n_bad, ("align_flat", name, p, st, n_bad, first)


# ---- the boundary of the fast variant's proof -----------------------------
@pytest.mark.parametrize("row", K.boundary_cases(), ids=lambda r: r["name"])
def test_boundary_rows_both_sides_of_the_proof(sw, sw_oracle_lib, golden, row, monkeypatch):
    b, p = row["batch"], row["params"]
    n1max, n2max = Z.maxima(b)
    for st in row["strategies"]:
        monkeypatch.delenv("HC_SW_GENERIC", raising=False)
        assert dp_variant(sw, p, st, n1max, n2max) == int(Z.fast_ok(p, st, n1max, n2max)) == int(row["fast"])
        got = run_batch(sw, b, p, st)
        g_off, g_cig = golden[f"boundary_{row['name']}_{st}"]
        n_bad, first = differing(got[:2], (g_off, g_cig))
        assert not n_bad, ("golden", row["name"], st, n_bad, first)
        want = sw_oracle_lib.batch(b, p, st, nthreads=8) + (sw_oracle_lib.scores(b, p, st),)
        n_bad, first = differing(got, want)
        assert not n_bad, ("oracle", row["name"], st, n_bad, first)
        if row["fast"]:
            monkeypatch.setenv("HC_SW_GENERIC", "1")
            assert dp_variant(sw, p, st, n1max, n2max) == 0
            n_bad, first = differing(run_batch(sw, b, p, st), got)
            assert not n_bad, ("generic", row["name"], st, n_bad, first)


# ---- order ----------------------------------------------------------------
def test_small_batches_after_a_large_one_in_the_workspace(sw, sw_oracle_lib):
    """hc_sw_align_flat borrows one grow-only workspace: after W3 of 4 regions
    it holds that batch's backtrack words, descriptors and results where the
    small batch's short last stripes write nothing."""
    big = S.config("W3", 4)
    assert len(big["ref_len"]) == 256
    want_big = sw_oracle_lib.batch(big, nthreads=8)
    small = [(name, b, sw_oracle_lib.batch(b, nthreads=8)) for name, b in K.order_cases()]

    def check(name, b, want):
        n_bad, first = differing(sw.align_flat(b), want)
        assert not n_bad, (name, n_bad, first)

    check("W3_4", big, want_big)
    for name, b, want in small:
        check(name, b, want)
    for name, b, want in reversed(small):
        check(name, b, want)
        check("W3_4 after " + name, big, want_big)
        check(name + " again", b, want)
