"""GPU parity of the quad prior table in its 16-byte form: a wide fp32
constant-gap wave reads the priors of four columns with one ds_read_b128 from a
table of NS = 40 quality rows of 16 float4 (256 bytes), entry = (prior of column
0, 1, 2, 3 of the group), physical column = pattern ^ (row & 15)
(seg_common.hpp fill_qtab, quad_row, quad_read, cell_tab). What that form can
get wrong, each compared bit for bit with the oracle (raw f32, rescue flag, raw
f64 of rescued pairs, loglik) through the flat call and a prepared batch at
forced block widths:
  - the order of the four floats: reads of all A against haps that repeat each
    of the 16 four-column patterns, at hap lengths whose left padding shifts
    the groups against column 0 and across the 32-column word boundary;
  - widths that end in a half group (62, 50, 34: 16 bytes read, .x and .y used);
  - the swizzle: qualities drawn per row from all NS values, so the lanes of a
    wave sit on table rows with every value of row & 15, rows 16-39 included,
    where the nibble wraps;
  - window edges: spans of exactly NS and of NS + 1 (pair table) in one launch,
    windows that start at quality 0 and that end at 127;
  - rows outside a read: reads of 1-3 rows between reads whose qualities lie
    far outside the window, which the unclamped prefetch sees.
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

NS = 40            # seg_common.hpp kQuadRows
LO = 33 + 2        # Phred 2..41: bytes 35..74, exactly NS values
H_SET = [33, 34, 35, 36, 37, 63, 64, 65, 66, 67, 68, 127, 128, 129, 130, 253, 500]
R_SET = [1, 2, 50, 101]
CAPS = [64, 62, 60, 50, 36, 34]   # 62, 50, 34: a half group at the block's end
ONE_HOT = [8, 4, 2, 1]
PATTERNS = ONE_HOT + [p for p in range(16) if p not in ONE_HOT]   # 16 * 17 * 4 = 1 088 pairs


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


def pattern_bases(p, H, R):
    """A read of all A against a hap that repeats the four-column pattern p of A
    (match) and C: with the paddings of H_SET every pattern meets every group
    position and every element of the 16 bytes."""
    unit = bytes(b"A"[0] if p >> (3 - j) & 1 else b"C"[0] for j in range(4))
    return np.full(R, ord("A"), np.uint8), np.frombuffer(unit * (H // 4 + 1), np.uint8)[:H].copy()


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
    """span: NS, or "mixed" (NS and NS + 1 by turns: quad and pair-table waves)."""
    rng = np.random.default_rng(41)
    pairs = []
    for p in PATTERNS:
        for H in H_SET:
            for R in R_SET:
                k = len(pairs)
                sp = (NS + (k >> 2 & 1)) if span == "mixed" else span   # by turns over (p, H): every R has both
                rs, hap = pattern_bases(p, H, R)
                pairs.append(pair(rs, quals(R, lo, sp, rng, k), hap))
    return W.from_pairs(pairs)


def all_rows_batch():
    """Pairs of many shapes, so the lanes of a wave sit on different rows, each
    row's quality uniform over all NS values of the window: within one wave the
    table rows take every value of row & 15, from rows 0-15 and from 16-39. A
    read is a stretch of its hap with two substitutions, so its likelihood stays
    far above the fp32 underflow (a random read of 40 rows and more sums to 0,
    whatever the priors) while the cells off its diagonal meet random patterns."""
    rng = np.random.default_rng(43)
    pairs = []
    for k in range(600):
        R = int(rng.integers(NS, 120))
        H = int(rng.integers(R, 400))
        hap = W.ACGT[rng.integers(0, 4, H)]
        o = int(rng.integers(0, H - R + 1))
        rs = hap[o:o + R].copy()
        rs[rng.choice(R, 2, replace=False)] = W.ACGT[rng.integers(0, 4, 2)]
        q = rng.permutation(np.concatenate([np.arange(NS), rng.integers(0, NS, R - NS)]))   # every row of the table
        pairs.append(pair(rs, (q + LO).astype(np.uint8), hap))
    return W.from_pairs(pairs)


def outside_rows_batch():
    """Reads of 1, 2, 3 rows with qualities in a window of NS bytes, each between
    reads whose qualities lie far outside it (bytes 33 and 126): the rows a short
    read prefetches past its end are its neighbours'."""
    rng = np.random.default_rng(47)
    pairs = []
    for k in range(360):
        H = [34, 40, 62, 64, 66, 130, 200][k % 7]
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


BATCHES = {
    "patterns": lambda: pattern_batch(LO, NS),          # Phred 2..41: every wave takes the quad table
    "mixed": lambda: pattern_batch(LO, "mixed"),        # spans of NS and NS + 1 in one launch
    "from_0": lambda: pattern_batch(128, NS),           # window starting at byte & 127 = 0
    "to_127": lambda: pattern_batch(128 - NS, NS),      # window ending at 127
    "all_rows": all_rows_batch,
    "outside": outside_rows_batch,
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


@pytest.mark.parametrize("name", ["patterns", "mixed", "from_0", "to_127", "all_rows"])
def test_batches_span_what_they_claim(batch, name):
    """Every read of two rows or more holds both ends of its window; the
    all_rows reads hold every one of its NS qualities."""
    b, ref = batch
    if name == "all_rows":   # the fp32 sums carry the priors: none underflows into the rescue
        assert not ref["rescued"].any() and (ref["raw_f32"] > 0).all()
    lo = {"from_0": 128, "to_127": 128 - NS}.get(name, LO)
    q, off, R = b["q"].astype(np.int64), b["read_off"], b["R"]
    spans = set()
    for o, r in zip(off, R):
        if r >= 2:
            v = (q[o:o + r] - lo) & 255
            assert v.min() == 0
            spans.add(int(v.max()) + 1)
            if name == "all_rows":
                assert len(set(v.tolist())) == NS
    assert spans == ({NS, NS + 1} if name == "mixed" else {NS})
    if name in ("from_0", "to_127"):
        assert (q & 127).min() == (0 if name == "from_0" else 128 - NS)
        assert (q & 127).max() == (NS - 1 if name == "from_0" else 127)


@pytest.mark.parametrize("name", ["patterns"])
@pytest.mark.parametrize("cap", CAPS)
def test_element_order_of_every_pattern(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")


@pytest.mark.parametrize("name", ["mixed", "from_0", "to_127"])
@pytest.mark.parametrize("cap", CAPS)
def test_window_edge(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")


@pytest.mark.parametrize("name", ["all_rows"])
@pytest.mark.parametrize("cap", CAPS)
def test_lanes_on_every_swizzle_of_all_rows(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")


@pytest.mark.parametrize("name", ["outside"])
@pytest.mark.parametrize("cap", CAPS)
def test_rows_outside_a_read(engine, batch, monkeypatch, name, cap):
    monkeypatch.setenv("HC_PHMM_SEG_CAP", str(cap))
    run_both(engine, *batch, f"{name} cap={cap}")
