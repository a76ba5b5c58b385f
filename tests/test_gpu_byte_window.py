"""GPU parity of the quad prior table in its byte form: a wide fp32 constant-gap
wave keeps its match window spread in LDS, one byte per group of four columns
(seg_spread.hpp), forms a group's table address as base2 ^ byte and reads the
priors from the workgroup's table of 64 quality rows, the quality bytes 33 .. 96
(Phred 0 .. 63), row = byte & 63 (seg_common.hpp fill_shared_tabs, quad_base2,
win_byte, cell_tab; lane_kernel.hip phmm_seg_kernel). Everything is compared bit
for bit with the oracle (raw f32, rescue flag, raw f64 of rescued pairs, loglik)
through the flat call and a prepared batch:
  - every even table width 34 .. 64 as the only width of its batch (the plan
    is checked on the CPU), the widths that end in a half group among them;
    haps of one block and of two and three, with and without padding left of
    column 1; reads of 1, 2, 3 rows (the prefetch edges) and of 40;
  - Phred 0 and 63 in every read (rows 33 and 32 of the table, where the row
    index wraps), binned qualities {2, 12, 23, 37}, reads with Ns (the fifth
    read code), and reads with a quality outside the table (Phred 64 and more,
    and a byte below 33), whose waves must take the pair table;
  - hap lengths of 500 and others that are no multiple of the width;
  - launches of 1, kSegWPB + 1 and 2 kSegWPB - 1 waves (a last workgroup with
    waves missing at the fill's barrier), and a workgroup that holds a quad
    wave beside a generic-path wave and a narrow wave.
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import hcphmm
import packing_cases as P
import workloads as W

WPB = 4                                  # lane_kernel.hip HC_SEG_WPB
WIDTHS = list(range(34, 65, 2))          # seg_common.hpp kQuadMinWidth .. kQuadMaxWidth
R_SET = [1, 2, 3, 40]
BINS = np.array([2, 12, 23, 37])
_cache = {}


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


def phred(R, rng, k, kind):
    """Phred qualities of a read. "ends": uniform over 0 .. 63 with both ends in
    the read (a one-row read takes one end, by turns); "bins": the four binned values."""
    if kind == "bins":
        return BINS[rng.integers(0, 4, R)]
    q = rng.integers(0, 64, R)
    if R == 1:
        q[0] = 63 * (k & 1)
    else:
        i, j = rng.choice(R, 2, replace=False)
        q[i], q[j] = 0, 63
    return q


def pair(rs, q, hap, ins=W.GOP, dels=W.GOP):
    n = len(rs)
    return (rs.tobytes(), np.asarray(q, np.uint8).tobytes(), np.full(n, ins, np.uint8).tobytes(),
            np.full(n, dels, np.uint8).tobytes(), np.full(n, W.GCP, np.uint8).tobytes(), hap.tobytes())


def bases(R, H, rng, k):
    """By turns a stretch of the hap with up to two substitutions (a likelihood
    far above the fp32 underflow) and a random read (long ones are rescued);
    every fifth read carries Ns."""
    hap = W.ACGT[rng.integers(0, 4, H)]
    if k & 1 and R <= H:
        o = int(rng.integers(0, H - R + 1))
        rs = hap[o:o + R].copy()
        rs[rng.integers(0, R, 2)] = W.ACGT[rng.integers(0, 4, 2)]
    else:
        rs = W.ACGT[rng.integers(0, 4, R)]
        hap[rng.random(H) < 0.4] = rs[0]   # enough matches for every four-column pattern
    if k % 5 == 0:
        rs = rs.copy()
        rs[rng.integers(0, R, max(1, R // 8))] = ord("N")
    return rs, hap


def width_haps(w):
    """Hap lengths that take blocks of w columns under a width cap of w: one
    block, two and three, each full and with one or two columns of padding."""
    return [w, w - 1, 2 * w, 2 * w - 1, 3 * w - 2]


def width_batch(w):
    rng = np.random.default_rng(1000 + w)
    pairs = []
    for rep in range(3):
        for H in width_haps(w):
            for R in R_SET:
                for kind in ("ends", "bins"):
                    k = len(pairs)
                    rs, hap = bases(R, H, rng, k)
                    pairs.append(pair(rs, phred(R, rng, k, kind) + 33, hap))
    # Qualities outside the table, each in a wave of eligible reads: Phred 64,
    # Phred 94 (byte 127) and a byte below Phred 0.
    for byte in (97, 127, 20):
        rs, hap = bases(40, 2 * w, rng, 1)
        q = phred(40, rng, 0, "ends") + 33
        q[7] = byte
        pairs.append(pair(rs, q, hap))
    return W.from_pairs(pairs)


def long_batch():
    rng = np.random.default_rng(71)
    pairs = []
    for H in (500, 500, 129, 200, 253, 333):
        for R in R_SET + [101]:
            for kind in ("ends", "bins"):
                k = len(pairs)
                rs, hap = bases(R, H, rng, k)
                pairs.append(pair(rs, phred(R, rng, k, kind) + 33, hap))
    return W.from_pairs(pairs)


def waves_batch(n_waves):
    """n_waves full waves of 64 one-block pairs at width 64, all quad waves."""
    rng = np.random.default_rng(80 + n_waves)
    pairs = []
    for k in range(64 * n_waves):
        rs, hap = bases(12, 64, rng, k)
        pairs.append(pair(rs, phred(12, rng, k, "ends") + 33, hap))
    return W.from_pairs(pairs)


def mixed_workgroup_batch():
    """Four waves, one workgroup: 64 pairs each of (width 64, unequal insertion
    and deletion gap qualities: the generic path), (width 64, quad), (width 64,
    quad, one row fewer) and (width 20, the carry select). The planner sorts by
    width, then steps, so each kind fills a wave of its own."""
    rng = np.random.default_rng(91)
    pairs = []
    for kind, (H, R, dels) in enumerate([(64, 14, 60), (64, 13, W.GOP), (64, 12, W.GOP), (20, 12, W.GOP)]):
        for k in range(64):
            rs, hap = bases(R, H, rng, k)
            pairs.append(pair(rs, phred(R, rng, k, "ends") + 33, hap, dels=dels))
    return W.from_pairs(pairs)


def get(name, make, oracle_lib):
    if name not in _cache:
        b = make()
        assert len(b["R"]) <= 600
        _cache[name] = (b, oracle_lib.pairs(b, nthreads=16))
    return _cache[name]


def plan_widths(b):
    """Block widths of the dry-run plan (no GPU) of a batch, one per wave."""
    return P.plan(P.bind(hcphmm.lib()), b)[3][:, 3]


def run_both(engine, b, ref, what, n_waves=None):
    assert_same(engine.pairs(b), ref, f"{what} flat")
    bt = engine.Batch(b)
    bt.run()
    res, st = bt.results(), bt.stats()
    bt.close()
    assert st.n_seg_waves > 0
    if n_waves is not None:
        assert st.n_seg_waves == n_waves
    assert_same(res, ref, f"{what} batch")


@pytest.mark.parametrize("w", WIDTHS)
def test_width_batches_plan_one_width_and_hold_the_qualities(monkeypatch, w):
    """CPU: the plan of a width's batch has that width only, and the batch holds
    what the GPU test claims (both table ends, bins, Ns, qualities outside)."""
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(w))
    b = width_batch(w)
    assert set(plan_widths(b).tolist()) == {w}
    q = b["q"].astype(np.int64) - 33
    ends = [(q[o:o + r].min(), q[o:o + r].max()) for o, r in zip(b["read_off"], b["R"]) if r >= 2]
    assert (0, 63) in ends and (2, 37) in ends
    assert {64, 94, -13} <= set(q.tolist()) and (b["rs"] == ord("N")).any()
    assert set(b["R"].tolist()) == set(R_SET)
    assert set(b["H"].tolist()) == set(width_haps(w))


def test_wave_count_batches_plan_what_they_claim(monkeypatch):
    """CPU: the workgroup-sharing batches plan 1, WPB + 1, 2 WPB - 1 waves of
    width 64, and the mixed workgroup four waves of widths 64, 64, 64, 20."""
    monkeypatch.setenv("HC_PHMM_SEG_CAP", "64")
    for n in (1, WPB + 1, 2 * WPB - 1):
        assert plan_widths(waves_batch(n)).tolist() == [64] * n
    b = mixed_workgroup_batch()
    pairs, order, n_seg, waves = P.plan(P.bind(hcphmm.lib()), b)
    w = waves[np.argsort(waves[:, 0], kind="stable")]
    assert w[:, 3].tolist() == [64, 64, 64, 20] and w[:, 4].tolist() == [64] * 4
    assert w[:, 1].tolist() == [14, 13, 12, 12]   # each kind in a wave of its own


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_every_width(engine, oracle_lib, monkeypatch, w):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(w))
    run_both(engine, *get(f"w{w}", lambda: width_batch(w), oracle_lib), f"width {w}")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [64, 50, 34])
def test_long_haps(engine, oracle_lib, monkeypatch, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    b, ref = get("long", long_batch, oracle_lib)
    assert 500 in b["H"] and plan_widths(b).max() >= 34   # (a cap of 34 leaves the shorter haps at 32)
    run_both(engine, b, ref, f"long haps cap={cap}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_waves", [1, WPB + 1, 2 * WPB - 1])
def test_wave_counts_around_a_workgroup(engine, oracle_lib, monkeypatch, n_waves):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", "64")
    run_both(engine, *get(f"n{n_waves}", lambda: waves_batch(n_waves), oracle_lib), f"{n_waves} waves", n_waves)


@pytest.mark.gpu
def test_workgroup_of_quad_generic_and_narrow_waves(engine, oracle_lib, monkeypatch):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", "64")
    run_both(engine, *get("mixed", mixed_workgroup_batch, oracle_lib), "mixed workgroup", 4)
