"""GPU parity of the quad prior table: wide fp32 constant-gap waves read a row's
priors four columns per address from an LDS table of NS = 40 consecutive
qualities, indexed by the row's quality and four match bits, with the column
swizzled by the table row (seg_common.hpp fill_qtab, quad_row, quad_addr); a
wave whose reads span more qualities keeps the pair table. These batches hold
what that can get wrong: each of the 16 four-column patterns at every group
position, hap lengths whose left padding shifts the groups against column 0 and
the 32-column word boundary, widths that end in a half group, quality windows
of exactly NS bytes (at the table's ends too) and of NS + 1, both kinds in one
launch, prefetched rows with qualities outside the window, and lanes of a wave
on rows whose swizzle differs. Everything is compared bit for bit with the
oracle, through the flat call and a prepared batch, at forced block widths.
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

NS = 40            # seg_common.hpp kQuadRows
LO = 33 + 2        # Phred 2..41: bytes 35..74, exactly NS values
H_SET = [33, 34, 35, 36, 37, 63, 64, 65, 66, 67, 68, 127, 128, 129, 130, 253, 500]
R_SET = [1, 2, 50, 101]
CAPS = [64, 62, 60, 36, 34]   # 62: half group at the block's end; 34: one half group in the second word
KINDS = [f"p{p:x}" for p in range(16)] + ["n_cols", "n_rows"]   # 18 * 17 * 4 = 1 224 pairs


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


def bases(kind, H, R, rng):
    """(read, hap). pX: the read is all A and the hap repeats the four-column
    pattern X of A (match) and C, so with the paddings of H_SET every pattern
    meets every group position; else random bases with N columns or N rows."""
    if kind[0] == "p":
        p = int(kind[1], 16)
        unit = bytes(b"A"[0] if p >> (3 - j) & 1 else b"C"[0] for j in range(4))
        return np.full(R, ord("A"), np.uint8), np.frombuffer(unit * (H // 4 + 1), np.uint8)[:H].copy()
    rs, hap = W.ACGT[rng.integers(0, 4, R)], W.ACGT[rng.integers(0, 4, H)]
    if kind == "n_rows":     # read code 4: the row's window is all ones
        rs[::3] = ord("N")
    else:                    # those columns match on every row
        hap[np.arange(H) % 7 % 3 == 0] = ord("N")
    return rs, hap


def quals(R, lo, span, rng, k):
    """Per-row draws from the `span` consecutive bytes from `lo` (mod 256), both
    ends in the read (a one-row read takes one end, by turns)."""
    q = rng.integers(0, span, R)
    if R == 1:
        q[0] = (span - 1) * (k & 1)
    else:
        i, j = rng.choice(R, 2, replace=False)
        q[i], q[j] = 0, span - 1
    return ((q + lo) & 255).astype(np.uint8)


def pair(rs, q, hap):
    g = np.full(len(rs), W.GOP, np.uint8)
    return (rs.tobytes(), q.tobytes(), g.tobytes(), g.tobytes(), np.full(len(rs), W.GCP, np.uint8).tobytes(),
            hap.tobytes())


def pattern_batch(lo, span):
    """span: NS, NS + 1, or "mixed" (the pairs alternate between the two)."""
    rng = np.random.default_rng(23)
    pairs = []
    for kind in KINDS:
        for H in H_SET:
            for R in R_SET:
                k = len(pairs)
                sp = (NS + (k >> 2 & 1)) if span == "mixed" else span   # by turns over (kind, H): every R has both
                rs, hap = bases(kind, H, R, rng)
                pairs.append(pair(rs, quals(R, lo, sp, rng, k), hap))
    return W.from_pairs(pairs)


def outside_rows_batch():
    """Reads of 1, 2, 3 rows with qualities in a window of NS bytes, each between
    reads whose qualities lie far outside it (bytes 33 and 126): the rows a short
    read prefetches past its end are its neighbours'."""
    rng = np.random.default_rng(29)
    pairs = []
    for k in range(360):
        H = [34, 40, 64, 66, 130, 200][k % 6]
        if k & 1:
            R = int(rng.integers(4, 12))
            q = np.full(R, 33 if k & 2 else 126, np.uint8)
        else:
            R = 1 + (k >> 1) % 3
            q = quals(R, 70, NS, rng, k >> 1)
        rs, hap = W.ACGT[rng.integers(0, 4, R)], W.ACGT[rng.integers(0, 4, H)]
        hap[rng.random(H) < 0.5] = rs[0]   # enough matches for every pattern
        pairs.append(pair(rs, q, hap))
    return W.from_pairs(pairs)


def swizzle_batch():
    """Pairs of many shapes, so the lanes of a wave sit on different rows, with
    qualities that differ in bits 1-4 from row to row: the XOR nibble differs per
    lane in every step."""
    rng = np.random.default_rng(31)
    pairs = []
    for k in range(500):
        H, R = int(rng.integers(34, 400)), int(rng.integers(5, 80))
        rs, hap = W.ACGT[rng.integers(0, 4, R)], W.ACGT[rng.integers(0, 4, H)]
        q = (LO + (rng.integers(0, 16, R) << 1) + (rng.integers(0, 2, R) if k & 1 else 0)).astype(np.uint8)
        pairs.append(pair(rs, q, hap))
    return W.from_pairs(pairs)


BATCHES = {
    "window": lambda: pattern_batch(LO, NS),            # Phred 2..41: every wave takes the quad table
    "wider": lambda: pattern_batch(LO, NS + 1),         # every read spans NS + 1: every wave falls back
    "mixed": lambda: pattern_batch(LO, "mixed"),        # waves of either kind in one launch
    "from_0": lambda: pattern_batch(128, NS),           # window starting at byte & 127 = 0
    "to_127": lambda: pattern_batch(128 - NS, NS),      # window ending at 127
    "outside": outside_rows_batch,
    "swizzle": swizzle_batch,
}
_cache = {}


@pytest.fixture
def batch(request, oracle_lib):
    """A batch and its oracle results (computed once, shared by the widths)."""
    name = request.node.callspec.params["name"]
    if name not in _cache:
        b = BATCHES[name]()
        assert len(b["R"]) <= 3000
        _cache[name] = (b, oracle_lib.pairs(b, nthreads=16))
    return _cache[name]


def run_both(engine, b, ref, what):
    assert_same(engine.pairs(b), ref, f"{what} flat")
    bt = engine.Batch(b)
    bt.run()
    res, st = bt.results(), bt.stats()
    bt.close()
    assert st.n_seg_waves > 0
    assert_same(res, ref, f"{what} batch")


@pytest.mark.parametrize("name", ["window", "wider", "mixed", "from_0", "to_127"])
def test_batches_span_what_they_claim(batch, name):
    """Every read of two rows or more holds both ends of its window."""
    b, _ = batch
    lo = {"from_0": 128, "to_127": 128 - NS}.get(name, LO)
    q, off, R = b["q"].astype(np.int64), b["read_off"], b["R"]
    spans = set()
    for o, r in zip(off, R):
        if r >= 2:
            v = (q[o:o + r] - lo) & 255
            assert v.min() == 0
            spans.add(int(v.max()) + 1)
    assert spans == {"wider": {NS + 1}, "mixed": {NS, NS + 1}}.get(name, {NS})
    if name in ("from_0", "to_127"):
        assert (q & 127).min() == (0 if name == "from_0" else 128 - NS)
        assert (q & 127).max() == (NS - 1 if name == "from_0" else 127)


@pytest.mark.parametrize("name", ["window"])
@pytest.mark.parametrize("cap", CAPS)
def test_every_pattern_at_every_group_position(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")


@pytest.mark.parametrize("name", ["wider", "mixed", "from_0", "to_127"])
@pytest.mark.parametrize("cap", CAPS)
def test_window_edge(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")


@pytest.mark.parametrize("name", ["outside"])
@pytest.mark.parametrize("cap", CAPS)
def test_rows_outside_a_read(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")


@pytest.mark.parametrize("name", ["swizzle"])
@pytest.mark.parametrize("cap", CAPS)
def test_lanes_on_rows_of_different_swizzle(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")
