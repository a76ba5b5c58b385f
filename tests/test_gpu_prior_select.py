"""GPU parity of the prior select: a row's match window is consumed MSB-first by
a shift chain (seg_common.hpp prior_next: add with carry-out, then a select on
the carry), so these batches hold the windows where such a chain can go wrong —
all ones, all zeros, alternating bits, 'N' rows and columns — at hap lengths
around the 32-column word boundaries and at forced block widths, bit for bit
against the oracle. Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

PATTERNS = ["ones", "zeros", "alt", "n_rows", "n_cols"]
H_SET = [1, 2, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129, 500]
R_SET = [1, 2, 50, 101]
REPS = 4   # quality draws per (pattern, H, R): 5 * 13 * 4 * 4 = 1 040 pairs


def assert_same(res, ref, what=""):
    """Bit-exact: raw f32, rescue decision, raw f64 of rescued pairs, log10 result."""
    r32 = res["raw_f32"].view(np.uint32) != ref["raw_f32"].view(np.uint32)
    assert not r32.any(), f"{what}: {r32.sum()} raw_f32 mismatches, first {np.nonzero(r32)[0][:10]}"
    assert np.array_equal(res["rescued"], ref["rescued"]), what
    m = ref["rescued"].astype(bool)
    r64 = res["raw_f64"][m].view(np.uint64) != ref["raw_f64"][m].view(np.uint64)
    assert not r64.any(), f"{what}: {r64.sum()} raw_f64 mismatches"
    ll = res["loglik"].view(np.uint64) != ref["loglik"].view(np.uint64)
    assert not ll.any(), f"{what}: {ll.sum()} loglik mismatches"


def pattern_pair(pattern, H, R, rng):
    """(read bases, hap bases) whose match windows follow `pattern`."""
    acgt = W.ACGT
    if pattern == "ones":       # every column of every row matches
        return np.full(R, ord("A"), np.uint8), np.full(H, ord("A"), np.uint8)
    if pattern == "zeros":      # no column of any row matches
        return np.full(R, ord("A"), np.uint8), np.full(H, ord("C"), np.uint8)
    if pattern == "alt":        # 1010... in every row
        return np.full(R, ord("A"), np.uint8), np.frombuffer(b"AC" * (H // 2 + 1), np.uint8)[:H].copy()
    rs, hap = acgt[rng.integers(0, 4, R)], acgt[rng.integers(0, 4, H)]
    if pattern == "n_rows":     # read code 4: the row's window is all ones
        rs[::3] = ord("N")
    else:                       # n_cols: those columns match on every row
        hap[np.arange(H) % 7 % 3 == 0] = ord("N")
    return rs, hap


def per_base_gaps(b, seed):
    """Per-base gap qualities: the generic cell path (as test_narrow_seg_widths)."""
    rng = np.random.default_rng(seed)
    n = len(b["ins"])
    b["ins"][:] = rng.integers(33 + 5, 33 + 60, n, dtype=np.uint8)
    b["dels"][:] = rng.integers(33 + 5, 33 + 60, n, dtype=np.uint8)
    b["gcp"][:] = rng.integers(33 + 5, 33 + 30, n, dtype=np.uint8)
    return b


def build(gaps, h_set=H_SET, r_set=R_SET, patterns=PATTERNS, reps=REPS, seed=7):
    rng = np.random.default_rng(seed)
    pairs = []
    for pat in patterns:
        for H in h_set:
            for R in r_set:
                for _ in range(reps):
                    rs, hap = pattern_pair(pat, H, R, rng)
                    q = (rng.integers(10, 41, R, dtype=np.uint8) + 33).astype(np.uint8)
                    g = np.full(R, W.GOP, np.uint8)
                    pairs.append((rs.tobytes(), q.tobytes(), g.tobytes(), g.tobytes(),
                                  np.full(R, W.GCP, np.uint8).tobytes(), hap.tobytes()))
    b = W.from_pairs(pairs)
    return per_base_gaps(b, seed + 1) if gaps == "per_base" else b


_cache = {}


@pytest.fixture
def windows(request, oracle_lib):
    """The pattern batch of one cell path and its oracle results (computed once)."""
    gaps = request.node.callspec.params["gaps"]
    if gaps not in _cache:
        b = build(gaps)
        assert len(b["R"]) <= 3000
        _cache[gaps] = (b, oracle_lib.pairs(b, nthreads=16))
    return _cache[gaps]


@pytest.mark.parametrize("gaps", ["eq", "per_base"])
@pytest.mark.parametrize("cap", [64, 34, 8])
def test_window_patterns_at_forced_widths(engine, windows, monkeypatch, gaps, cap):
    """fp32 pass at block widths up to `cap` (34: the switch from the first
    window word to the second comes with two columns left; 8: one byte of the
    first word), both cell paths, flat call and prepared batch."""
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    b, ref = windows
    assert_same(engine.pairs(b), ref, f"cap={cap}/{gaps} flat")
    bt = engine.Batch(b)
    bt.run()
    res, st = bt.results(), bt.stats()
    bt.close()
    assert st.n_seg_waves > 0
    assert_same(res, ref, f"cap={cap}/{gaps} batch")


@pytest.mark.parametrize("gaps", ["eq", "per_base"])
def test_window_patterns_fp64_on_every_pair(engine, windows, gaps):
    """The pattern pairs that underflow in fp32, alone: every pair of the batch
    takes the fp64 path (as test_golden_f64_path_on_every_pair forces it)."""
    b, ref = windows
    idx = np.nonzero(ref["rescued"].astype(bool))[0]
    assert len(idx) > 100
    sub = W.subset(b, idx)
    res = engine.pairs(sub)
    assert res["rescued"].all()
    assert_same(res, {k: ref[k][idx] for k in ("raw_f32", "rescued", "raw_f64", "loglik")}, f"fp64/{gaps}")


def test_window_patterns_fp64_chained(engine, oracle_lib, monkeypatch):
    """64-lane fp64 pairs chained through the same lanes (HC_PHMM_CHAIN_TAIL=0,
    more than two waves per SIMD, as test_fp64_long_haps_many_waves
    [long-haps-chained]): the match windows change between the pairs of one
    wave, and neighbouring pairs here have different patterns."""
    monkeypatch.setenv("HC_PHMM_CHAIN_TAIL", "0")
    b = build("eq", h_set=[1025, 1056, 1057, 1500, 2047, 2048], r_set=[50, 101],
              patterns=["zeros", "alt", "n_rows", "n_cols"], reps=62, seed=9)
    # interleave the patterns, so that a chain's pairs differ
    perm = np.random.default_rng(3).permutation(len(b["R"]))
    b = W.subset(b, perm)
    assert 2500 < len(b["R"]) <= 3000
    ref = oracle_lib.pairs(b, nthreads=16)
    assert ref["rescued"].sum() > 2200   # more than two 64-lane waves per SIMD: the pass chains
    assert_same(engine.pairs(b), ref, "chained flat")
    bt = engine.Batch(b)
    bt.run()
    assert_same(bt.results(), ref, "chained batch")
    bt.close()
