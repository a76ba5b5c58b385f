"""What a Smith-Waterman batch exercises, stated on the expected side.

Plain Python and numpy; no GPU code is read. The CPU census tests and the GPU
edge tests both import it, so that a claim about an input ("this batch takes
the tall LDS layout", "this pair carries a 129-base interior deletion", "this
parameter row is just inside the fast variant's proof") is computed, not
believed.

* cigar_census / batch_census: from expected CIGAR strings.
* dp: the Gotoh recurrences of PairWiseSW.h MAIN_CODE (:4-38), row-wise in
  int64, with and without the MATRIX_MIN_CUTOFF max.
* fast_ok, row_slots, fslots, tall_layout: restatements of csrc/sw_engine.cpp
  and csrc/sw_kernels.hpp, for the expected side only.
"""
from __future__ import annotations

import re

import numpy as np

SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 9, 10, 11, 12
MIN_CUTOFF = -100000000          # MATRIX_MIN_CUTOFF (smithwaterman_common.h:50)
LOW_INIT = -(1 << 30)            # LOW_INIT_VALUE = INT32_MIN / 2 (:51)
STRIPE, GROUP = 64, 8

_ELEM = re.compile(r"(\d+)([MIDSR])")


# ---- CIGAR census ---------------------------------------------------------
def elements(cigar: str):
    el = [(int(n), op) for n, op in _ELEM.findall(cigar)]
    assert "".join(f"{n}{op}" for n, op in el) == cigar, cigar
    return el


def cigar_census(cigar: str) -> dict:
    """Longest interior I and D (an I or D with an M on both sides), the soft
    clips on either end, the element count, and where the end point lies: a
    trailing S means the scan stopped on the last row before the last column
    (PairWiseSW.h:254-262), otherwise it lies on the last column."""
    el = elements(cigar)
    ins = dele = 0
    for k in range(1, len(el) - 1):
        if el[k - 1][1] == "M" and el[k + 1][1] == "M":
            if el[k][1] == "I":
                ins = max(ins, el[k][0])
            elif el[k][1] == "D":
                dele = max(dele, el[k][0])
    lead = el[0][0] if el and el[0][1] == "S" else 0
    trail = el[-1][0] if len(el) > 1 and el[-1][1] == "S" else 0
    return dict(interior_i=ins, interior_d=dele, lead_s=lead, trail_s=trail, n_elems=len(el),
                end_on="row" if trail else "col")


def batch_census(cigars) -> dict:
    c = [cigar_census(x) for x in cigars]
    gap = [max(x["interior_i"], x["interior_d"]) for x in c]
    return dict(
        interior_i=max((x["interior_i"] for x in c), default=0),
        interior_d=max((x["interior_d"] for x in c), default=0),
        lead_s=max((x["lead_s"] for x in c), default=0),
        trail_s=max((x["trail_s"] for x in c), default=0),
        n_elems=max((x["n_elems"] for x in c), default=0),
        end_on_row=sum(x["end_on"] == "row" for x in c),
        end_on_col=sum(x["end_on"] == "col" for x in c),
        # pairs with a soft clip on either end and an interior gap of 64 or more
        clip_next_to_long_gap=sum((x["lead_s"] > 0 or x["trail_s"] > 0) and g >= 64 for x, g in zip(c, gap)),
    )


# ---- restatements of the host's layout and variant decisions --------------
def row_slots(n2max: int) -> int:
    return (n2max + 2 * STRIPE + 4 * GROUP + 3) & ~3


def fslots(n1max: int, n2max: int) -> int:
    return row_slots(n2max) if row_slots(n2max) > n1max + 1 else (n1max + 4) & ~3


def tall_layout(n1max: int, n2max: int) -> bool:
    """The last-column buffer, not the row buffer, sizes rowF / colC."""
    return n1max + 1 > row_slots(n2max)


def stripe_steps(n2: int) -> int:
    return (n2 + STRIPE + GROUP - 1) & ~(GROUP - 1)


def short_last_stripe(n1: int, n2: int) -> bool:
    """The fast DP ends a partial last stripe of r rows after n2 + r - 1 steps
    and writes no backtrack words past them (sw_kernels.hip, Ts < T)."""
    r = n1 % STRIPE
    return r != 0 and ((n2 + r + GROUP - 1) & ~(GROUP - 1)) < stripe_steps(n2)


def maxima(batch):
    return int(batch["ref_len"].max()), int(batch["alt_len"].max())


def fast_ok(params, overhang: int, n1max: int, n2max: int) -> bool:
    mt, mm, op, ex = (int(x) for x in params)
    M = max(n1max, n2max)
    bmin = bmax = 0
    if overhang in (INDEL, LEADING_INDEL):
        bmin = min(0, op, op + (M - 1) * ex)
        bmax = max(0, op, op + (M - 1) * ex)
    hlow = bmin + M * min(0, mt, mm)
    hhigh = bmax + M * max(0, mt, mm)
    if hlow < MIN_CUTOFF:
        return False
    v = max(-hlow, hhigh) + abs(op) + M * abs(ex) + abs(mt) + abs(mm)
    return v < (1 << 28)


def fast_ok_without_cutoff_clause(params, overhang, n1max, n2max) -> bool:
    """fast_ok with its `hlow < MATRIX_MIN_CUTOFF` clause removed: true for a
    row that the cutoff clause alone keeps out of the fast variant."""
    mt, mm, op, ex = (int(x) for x in params)
    M = max(n1max, n2max)
    bmin = bmax = 0
    if overhang in (INDEL, LEADING_INDEL):
        bmin = min(0, op, op + (M - 1) * ex)
        bmax = max(0, op, op + (M - 1) * ex)
    hlow = bmin + M * min(0, mt, mm)
    hhigh = bmax + M * max(0, mt, mm)
    return max(-hlow, hhigh) + abs(op) + M * abs(ex) + abs(mt) + abs(mm) < (1 << 28)


# ---- the DP, row-wise in int64 --------------------------------------------
def _boundary(overhang, op, ex, x):
    """H(0, x) and H(x, 0) (PairWiseSW.h:188-197); H(0, 0) = 0 (:80)."""
    x = np.asarray(x, np.int64)
    if overhang in (INDEL, LEADING_INDEL):
        return np.where(x > 0, op + (x - 1) * ex, 0)
    return np.zeros_like(x)


def _sweep(params, overhang, s1, s2, cutoff: bool):
    mt, mm, op, ex = (int(x) for x in params)
    a = np.frombuffer(s1, np.uint8)
    b = np.frombuffer(s2, np.uint8)
    n1, n2 = len(a), len(b)
    cols = np.arange(n2 + 1, dtype=np.int64)
    Hp = _boundary(overhang, op, ex, cols)            # row 0
    Fp = np.full(n2 + 1, LOW_INIT, np.int64)          # F(0, j) (:198)
    jx = cols[1:] * ex
    lowest = None
    bound = False
    last_col = np.zeros(n1 + 1, np.int64)
    last_col[0] = Hp[n2]
    for i in range(1, n1 + 1):
        h0 = int(_boundary(overhang, op, ex, i))
        d = Hp[:-1] + np.where(b == a[i - 1], mt, mm)
        if cutoff:
            bound = bound or bool((d < MIN_CUTOFF).any())
            d = np.maximum(d, MIN_CUTOFF)
        F = np.maximum(Fp[1:] + ex, Hp[1:] + op)
        T = np.maximum(d, F)                           # H(i, j) but for E
        H = np.empty(n2 + 1, np.int64)
        H[0] = h0
        if op <= ex:
            # E(i, j) = max(H(i, j-1) + open, E(i, j-1) + extend), E(i, 0) = LOW.
            # An H that is itself an E never opens a better gap than extending
            # that E (open <= extend), so H may be replaced by T in the
            # recurrence, which then unrolls into a running maximum.
            src = np.concatenate(([h0], T[:-1])) + op - cols[:-1] * ex     # column k opens: T'(k) + open - k * ex
            E = np.maximum(np.maximum.accumulate(src) + (cols[1:] - 1) * ex, LOW_INIT + jx)
            H[1:] = np.maximum(T, E)
        else:
            e = LOW_INIT
            for j in range(1, n2 + 1):
                e = max(int(H[j - 1]) + op, e + ex)
                H[j] = max(int(T[j - 1]), e)
        m = int(H[1:].min())
        lowest = m if lowest is None else min(lowest, m)
        last_col[i] = H[n2]
        Fp = np.concatenate(([LOW_INIT], F))
        Hp = H
    return dict(lowest=lowest, bound=bound, last_row=Hp.copy(), last_col=last_col)


def dp(params, overhang, s1: bytes, s2: bytes) -> dict:
    """The DP of one pair. `lowest_h` is the lowest H(i, j), i, j >= 1, of the
    recurrences without the cutoff max (what the fast variant computes);
    `bound` says whether H(i-1, j-1) + score fell below MATRIX_MIN_CUTOFF at any
    cell of the recurrences with it; `last_row` / `last_col` (index 0 = the
    boundary) and `score` are the reference's, with the cutoff; `n_best` counts
    the end-point candidates that hold the best score (PairWiseSW.h:201-226)."""
    free = _sweep(params, overhang, s1, s2, False)
    cut = _sweep(params, overhang, s1, s2, True)
    n1, n2 = len(s1), len(s2)
    cand = {(i, n2): int(cut["last_col"][i]) for i in range(1, n1 + 1)}
    if overhang in (SOFTCLIP, IGNORE):
        cand.update({(n1, j): int(cut["last_row"][j]) for j in range(1, n2 + 1)})
    best = max(cand.values())
    return dict(lowest_h=free["lowest"], lowest_h_cut=cut["lowest"], bound=cut["bound"],
                last_row=cut["last_row"], last_col=cut["last_col"], score=best,
                n_best=sum(v == best for v in cand.values()))
