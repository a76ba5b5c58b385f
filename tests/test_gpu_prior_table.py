"""GPU parity of the prior pair table: the fp32 constant-gap path reads a row's
priors two columns at a time from an LDS table indexed by the row's quality and
the two columns' match bits (seg_common.hpp ptab, cell_tab). These batches hold
what such a lookup can get wrong — each of the four two-column patterns at every
pair position of a block, hap lengths whose left padding splits a pair across
column 0 or moves the 32-column word boundary, every quality byte, lanes of one
wave on different table rows — at forced block widths, bit for bit against the
oracle, through the flat call and a prepared batch. Run on an MI355X:
pytest -m gpu."""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

PATTERNS = ["ones", "zeros", "alt10", "alt01", "random", "n_rows", "n_cols"]
H_SET = [1, 2, 3, 4, 31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 500]
R_SET = [1, 2, 50, 101]
REPS = 4   # quality draws per (pattern, H, R): 7 * 16 * 4 * 4 = 1 792 pairs


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
    a = np.full(R, ord("A"), np.uint8)
    if pattern == "ones":       # 11 at every pair of every row
        return a, np.full(H, ord("A"), np.uint8)
    if pattern == "zeros":      # 00
        return a, np.full(H, ord("C"), np.uint8)
    if pattern == "alt10":      # 1010...: 10 or 01 at every pair, by the padding's parity
        return a, np.frombuffer(b"AC" * (H // 2 + 1), np.uint8)[:H].copy()
    if pattern == "alt01":      # 0101...
        return a, np.frombuffer(b"CA" * (H // 2 + 1), np.uint8)[:H].copy()
    rs, hap = acgt[rng.integers(0, 4, R)], acgt[rng.integers(0, 4, H)]
    if pattern == "n_rows":     # read code 4: the row's window is all ones
        rs[::3] = ord("N")
    elif pattern == "n_cols":   # those columns match on every row
        hap[np.arange(H) % 7 % 3 == 0] = ord("N")
    return rs, hap


def accepted_quality_bytes(oracle_lib):
    """The quality bytes the oracle takes, found on the CPU: one short pair per
    byte value, accepted when the oracle returns a number for it."""
    rng = np.random.default_rng(5)
    pairs = []
    for v in range(256):
        rs, hap = W.ACGT[rng.integers(0, 4, 3)], W.ACGT[rng.integers(0, 4, 5)]
        g = np.full(3, W.GOP, np.uint8)
        pairs.append((rs.tobytes(), np.full(3, v, np.uint8).tobytes(), g.tobytes(), g.tobytes(),
                      np.full(3, W.GCP, np.uint8).tobytes(), hap.tobytes()))
    ref = oracle_lib.pairs(W.from_pairs(pairs), nthreads=4)
    return np.nonzero(~np.isnan(ref["loglik"]))[0].astype(np.uint8)


def per_base_gaps(b, seed):
    """Per-base gap qualities: the generic cell path (as test_gpu_prior_select)."""
    rng = np.random.default_rng(seed)
    n = len(b["ins"])
    b["ins"][:] = rng.integers(33 + 5, 33 + 60, n, dtype=np.uint8)
    b["dels"][:] = rng.integers(33 + 5, 33 + 60, n, dtype=np.uint8)
    b["gcp"][:] = rng.integers(33 + 5, 33 + 30, n, dtype=np.uint8)
    return b


def build(gaps, qbytes, seed=11):
    """Qualities are drawn per row, so the lanes of a wave read different table
    rows in the same step: the first half of the draws from the usual Phred
    10..40 (+33), the second from every accepted byte."""
    rng = np.random.default_rng(seed)
    pairs = []
    for pat in PATTERNS:
        for H in H_SET:
            for R in R_SET:
                for rep in range(REPS):
                    rs, hap = pattern_pair(pat, H, R, rng)
                    if rep < REPS // 2:
                        q = (rng.integers(10, 41, R, dtype=np.uint8) + 33).astype(np.uint8)
                    else:
                        q = qbytes[rng.integers(0, len(qbytes), R)]
                    g = np.full(R, W.GOP, np.uint8)
                    pairs.append((rs.tobytes(), q.tobytes(), g.tobytes(), g.tobytes(),
                                  np.full(R, W.GCP, np.uint8).tobytes(), hap.tobytes()))
    b = W.from_pairs(pairs)
    return per_base_gaps(b, seed + 1) if gaps == "per_base" else b


_cache = {}


@pytest.fixture
def tables(request, oracle_lib):
    """The pattern batch of one cell path and its oracle results (computed once)."""
    gaps = request.node.callspec.params["gaps"]
    if "qbytes" not in _cache:
        _cache["qbytes"] = accepted_quality_bytes(oracle_lib)
    qbytes = _cache["qbytes"]
    if gaps not in _cache:
        b = build(gaps, qbytes)
        assert len(b["R"]) <= 3000
        _cache[gaps] = (b, oracle_lib.pairs(b, nthreads=16))
    return _cache[gaps] + (qbytes,)


def run_both(engine, b, ref, what):
    assert_same(engine.pairs(b), ref, f"{what} flat")
    bt = engine.Batch(b)
    bt.run()
    res, st = bt.results(), bt.stats()
    bt.close()
    assert st.n_seg_waves > 0
    assert_same(res, ref, f"{what} batch")


@pytest.mark.parametrize("gaps", ["eq"])
def test_batch_covers_every_accepted_quality_byte(tables, gaps):
    """The oracle takes every byte (it uses q & 127), and the batch holds each,
    so every row of the table is read."""
    b, _, qbytes = tables
    assert len(qbytes) == 256
    assert np.isin(qbytes, b["q"]).all()
    assert len(np.unique(b["q"] & 127)) == 128


@pytest.mark.parametrize("gaps", ["eq"])
@pytest.mark.parametrize("cap", [64, 62, 34, 32, 8])
def test_pair_patterns_at_forced_widths(engine, tables, monkeypatch, gaps, cap):
    """fp32 pass at block widths up to `cap` (64 and 62: the widest blocks; 34:
    the narrowest that reads the table, one pair in the second window word; 32
    and 8: blocks that keep the select and take pm and px from the table's
    rows), flat call and prepared batch."""
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    b, ref, _ = tables
    run_both(engine, b, ref, f"cap={cap}/{gaps}")


@pytest.mark.parametrize("gaps", ["per_base"])
def test_per_base_gaps_take_the_select(engine, tables, gaps):
    """The same pairs with per-base gap qualities: the generic path, which keeps
    the carry select, unchanged."""
    b, ref, _ = tables
    run_both(engine, b, ref, "per_base")
