"""Batches and plan arithmetic shared by test_planner_packing.py (CPU) and
test_gpu_packing.py (GPU): the general host planner's segmented waves, read
back through the dry-run hooks (hcx_plan_pairs, hcx_dump_*)."""
import contextlib
import ctypes as C
import os

import numpy as np

import hcphmm
import workloads as W

WIDTHS = set(range(8, 65, 2))   # HC_SEG_WIDTHS (seg_common.hpp)


def batch(H, R, seed, subst=0.01, q_range=(10, 40)):
    """A flat batch with the given hap and read lengths (R <= H): reads drawn
    from their haps as workloads.generate does."""
    rng = np.random.default_rng(seed)
    H = np.asarray(H, np.int64)
    R = np.asarray(R, np.int64)
    assert (R <= H).all() and (R > 0).all()
    hap_off = np.concatenate([[0], np.cumsum(H[:-1])]).astype(np.int64)
    read_off = np.concatenate([[0], np.cumsum(R[:-1])]).astype(np.int64)
    tot_h, tot_r = int(H.sum()), int(R.sum())
    hap = rng.integers(0, 4, size=tot_h, dtype=np.uint8)
    start = np.floor(rng.random(len(H)) * (H - R + 1)).astype(np.int64)
    idx = np.arange(tot_r, dtype=np.int64) + np.repeat(hap_off + start - read_off, R)
    rd = hap[idx]
    sub = rng.random(tot_r) < subst
    rd[sub] = (rd[sub] + rng.integers(1, 4, size=int(sub.sum()), dtype=np.uint8)) % 4
    q = (rng.integers(q_range[0], q_range[1] + 1, size=tot_r, dtype=np.uint8) + 33).astype(np.uint8)
    return dict(read_off=read_off, R=R.astype(np.int32), hap_off=hap_off, H=H.astype(np.int32),
                rs=W.ACGT[rd], q=q, ins=np.full(tot_r, W.GOP, np.uint8), dels=np.full(tot_r, W.GOP, np.uint8),
                gcp=np.full(tot_r, W.GCP, np.uint8), hap=W.ACGT[hap])


@contextlib.contextmanager
def columns(cap, q=None):
    """Plan with at most `cap` columns per lane (q = 0: on ceil(H / cap) lanes
    per pair) through the planner's sweep switches, whatever its cost model
    would choose for so small a batch."""
    want = {"HC_PHMM_SEG_CAP": str(cap)}
    if q is not None:
        want["HC_PHMM_SEG_Q"] = str(q)
    old = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def one_bin(seed=11):
    """700 pairs of one width bin with nb = 2 ... 10 when planned under
    columns(50, 0): H = 100, 150, ..., 500 in turn (78 or 77 pairs each: neither
    divides 64), R in 40 ... 60."""
    rng = np.random.default_rng(seed)
    H = 100 + 50 * (np.arange(700) % 9)
    R = rng.integers(40, 61, 700)
    return batch(H, R, seed)


def two_widths(seed=12):
    """300 pairs straddling the step from two lanes to three: H = 100 ... 140
    in steps of 2, R in 20 ... 30. Under columns(64) that is two lanes of 50
    ... 64 columns up to H = 128 and three of 44 ... 48 above: a dozen widths
    of about 14 pairs each, so every width's last wave closes with lanes free."""
    rng = np.random.default_rng(seed)
    H = 100 + 2 * rng.integers(0, 21, 300)
    R = rng.integers(20, 31, 300)
    return batch(H, R, seed)


def low_quality_read(seed=13):
    """40 pairs of mixed nb, one of them (pair 17) a 200-base read of Phred-2
    qualities throughout. Low qualities alone leave its likelihood near
    1e-19, so every base also mismatches its hap: 1e-448, which underflows
    the fp32 sum, and its wave rescues it."""
    rng = np.random.default_rng(seed)
    H = 100 + 50 * (np.arange(40) % 9)
    R = rng.integers(40, 61, 40)
    H[17], R[17] = 450, 200
    b = batch(H, R, seed)
    o = int(b["read_off"][17])
    b["q"][o:o + 200] = 2 + 33
    swap = np.zeros(256, np.uint8)
    swap[list(b"ACGT")] = list(b"CATG")
    b["rs"][o:o + 200] = swap[b["rs"][o:o + 200]]
    return b


def bind(lib):
    lib.hcx_plan_pairs.restype = C.c_double
    lib.hcx_dump_sizes.argtypes = [C.c_void_p]
    lib.hcx_dump_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def plan(lib, b):
    """Dry-run plan of a flat batch on one modelled 256-CU device: the last
    part's (pairs, order, n_seg, waves); waves as rows of {slot0, rmax, rmin,
    ncols, npairs, nsteps}."""
    args, keep = hcphmm._flat_args(b)
    lib.hcx_plan_pairs(*args, C.c_int(256), C.c_int(1), C.c_int(1))
    sz = np.zeros(5, np.int64)
    lib.hcx_dump_sizes(sz.ctypes.data)
    n_pairs, n_order, n_seg, n_waves, grid = (int(x) for x in sz)
    pairs = np.zeros((max(n_pairs, 1), 4), np.int32)
    order = np.zeros(max(n_order, 1), np.int32)
    waves = np.zeros((max(n_waves, 1), 6), np.int32)
    lib.hcx_dump_plan(pairs.ctypes.data, order.ctypes.data, waves.ctypes.data)
    assert grid == 0
    return pairs[:n_pairs], order[:n_order], n_seg, waves[:n_waves]


def wave_table(pairs, order, n_seg, waves):
    """Per segmented slot, in slot order: (wave index, R, H, nb, steps), the
    waves sorted by slot0."""
    w = waves[np.argsort(waves[:, 0], kind="stable")]
    wid = np.repeat(np.arange(len(w)), w[:, 4])
    p = order[:n_seg]
    R = pairs[p, 1].astype(np.int64)
    H = pairs[p, 3].astype(np.int64)
    nb = -(-H // w[wid, 3])
    return w, wid, R, H, nb, R + nb - 1


def lane_stats(pairs, order, n_seg, waves):
    """(lane efficiency, empty-lane share) of a plan: useful cells, and the
    lanes no pair holds, over the swept lane-cells sum(64 * BC * nsteps)."""
    w, wid, R, H, nb, steps = wave_table(pairs, order, n_seg, waves)
    swept = float((64 * w[:, 3].astype(np.int64) * w[:, 5]).sum())
    lanes = np.bincount(wid, weights=nb, minlength=len(w))
    empty = float(((64 - lanes) * w[:, 3] * w[:, 5]).sum())
    return float((R * H).sum()) / swept, empty / swept
