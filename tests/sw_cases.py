"""Seeded Smith-Waterman case families for the batches and scores that the
region workloads and the edge grid of sw_workloads.py do not reach. Every
family is a list of named batches in the sw_workloads layout; what each one
exercises is computed by sw_census.py and asserted in test_sw_census.py.

layout_batches   batch maxima that size the DP kernel's LDS differently: tall
                 and narrow (the last-column buffer outgrows the row buffer),
                 a single column, a single row, and the 8-column word and
                 64-row stripe borders; an odd pair count each, so that the last
                 workgroup is partly filled at 2 and 4 waves.
gap_pairs        one long deletion or insertion between matching flanks, at
                 the lengths around the traceback's 64-cell runs, starting next
                 to the stripe borders, with unrelated alt ends (a soft clip on
                 either side of the gap), and in region-shaped sets.
boundary_cases   parameter rows just inside and just outside the proof that
                 lets the DP drop the MATRIX_MIN_CUTOFF max (sw_engine.cpp
                 fast_ok), on pairs whose H really goes down to the cutoff.
order_cases      small batches to run after a large one through the borrowed
                 workspace.

boundary_cases has one pair whose expected CIGAR carries an interior gap while
its own path runs within 5 % of the cutoff: under INDEL and LEADING_INDEL a
pair of unequal lengths must take a gap somewhere, and with matching flanks
around 982 mismatches it is an interior one (`...M1D...M`, path score about
-96e6). Under SOFTCLIP / IGNORE no such pair exists for these rows: a gap costs
50e6 to open, and clipping or running through the mismatches is always cheaper
than a gap that the alignment is free to avoid.

The row (1000, -99000, -1000000, -1000) under INDEL is outside fast_ok by its
cutoff clause alone, but the cutoff does not bind on it: with an open score of
-1e6 the DP walks round the mismatches with two giant gaps (`1003D1003I20M`),
and no H goes below -4.1e6. The rows that bind are (1000, -97000, -50000000,
-100000) under INDEL, whose border alone reaches -152e6 and which fast_ok's
int32 clause refuses as well, and (1000, -97000, -50000000, -1000) under INDEL
and LEADING_INDEL, which only the cutoff clause keeps out of the fast variant.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

import sw_workloads as S

GAP_LENGTHS = (63, 64, 65, 127, 128, 129, 200, 500)
FLANKS = ((40, 40), (10, 70), (64, 64))
STRIPE_STARTS = (60, 63, 64, 65, 70, 120, 127, 128, 129, 135)   # rows / columns before the gap

LAYOUT_MAXIMA = ((1023, 1), (1023, 8), (1023, 9), (600, 64), (65, 1), (1, 1), (1, 1024), (64, 1024), (200, 200))
LAYOUT_COUNTS = (5, 7, 9)


def _rand(rng, n):
    return S.ACGT[rng.integers(0, 4, n)]


# ---- layout ---------------------------------------------------------------
def _sizes(rng, top, mod, classes, k):
    """A size in [1, top] whose residue modulo `mod` is classes[k % 3] where
    such a size exists, any of the three classes otherwise."""
    want = [x for x in range(1, top + 1) if x % mod == classes[k % len(classes)]]
    if not want:
        want = [x for x in range(1, top + 1) if x % mod in classes] or [top]
    return int(want[int(rng.integers(0, len(want)))])


def _layout_pair(rng, n1, n2):
    r = S._window(rng, n1)
    if rng.random() < 0.5 and n2 <= n1:
        o = int(rng.integers(0, n1 - n2 + 1))
        a = S._mutate(rng, r[o:o + n2], 0.03, 0.0, 0.0)
    else:
        a = _rand(rng, n2)
    return r.tobytes(), a[:n2].tobytes()


def layout_pair_lists(seed=201):
    """[(name, [(ref, alt)])]: the maximal pair first, then pairs at and below
    the maxima with n1 % 64 in {0, 1, 63} and n2 % 8 in {0, 1, 7}."""
    rng = np.random.default_rng(seed)
    out = []
    for b, (N1, N2) in enumerate(LAYOUT_MAXIMA):
        pairs = [_layout_pair(rng, N1, N2)]
        for k in range(1, LAYOUT_COUNTS[b % 3]):
            n1 = _sizes(rng, N1, 64, (0, 1, 63), k)
            n2 = _sizes(rng, N2, 8, (0, 1, 7), k + k // 3)
            pairs.append(_layout_pair(rng, n1, n2))
        out.append((f"{N1}x{N2}", pairs))
    return out


def layout_batches(seed=201):
    return [(name, S.from_pairs(p)) for name, p in layout_pair_lists(seed)]


def layout_union(seed=201):
    """Every pair of layout_batches() in one tall-and-wide batch (maxima 1023 x
    1024), and name -> the pairs' indices in it."""
    pairs, where = [], {}
    for name, p in layout_pair_lists(seed):
        where[name] = list(range(len(pairs), len(pairs) + len(p)))
        pairs += p
    return S.from_pairs(pairs), where


# ---- long gaps ------------------------------------------------------------
def _gap_pair(rng, f1, L, f2, deletion, lead=0, trail=0):
    w = _rand(rng, f1 + L + f2)
    short = np.concatenate([w[:f1], w[f1 + L:]])
    ref, alt = (w, short) if deletion else (short, w)
    alt = np.concatenate([_rand(rng, lead), alt, _rand(rng, trail)])
    return ref.tobytes(), alt.tobytes()


def _gap_region(rng, n, haps):
    """One window of n bases and `haps` haplotypes, built like
    sw_workloads.regions(): hap 0 is the window, every other one carries the
    usual SNPs and one 60 to 300-base deletion or insertion."""
    w = S._window(rng, n)
    out = [(w.tobytes(), w.tobytes())]
    for _ in range(1, haps):
        x = S._mutate(rng, w, 0.01, 0.0, 0.0)
        if rng.random() < 0.5:
            L = int(rng.integers(60, min(300, len(x) - 80) + 1))
            p = int(rng.integers(40, len(x) - L - 40 + 1))
            x = np.concatenate([x[:p], x[p + L:]])
        else:
            L = int(rng.integers(60, min(300, S.MAX_LEN - len(x)) + 1))
            p = int(rng.integers(40, len(x) - 40 + 1))
            x = np.concatenate([x[:p], _rand(rng, L), x[p:]])
        out.append((w.tobytes(), x.tobytes()))
    return out


def _shared_ref_batch(pairs):
    """from_pairs, but pairs of one window share its bytes, as in regions()."""
    b = S.from_pairs(pairs)
    seen, refs, ro, off = {}, [], [], 0
    for r, _ in pairs:
        if r not in seen:
            seen[r] = off
            refs.append(np.frombuffer(r, np.uint8))
            off += len(r)
        ro.append(seen[r])
    b["refs"] = np.concatenate(refs)
    b["ref_off"] = np.array(ro, np.int64)
    return b


def gap_pairs(seed=202):
    """[(name, batch)]: flanks / stripes / clipped are one gap between matching
    flanks; region415 / region900 are region-shaped."""
    rng = np.random.default_rng(seed)
    flanks = [_gap_pair(rng, f1, L, f2, d) for L in GAP_LENGTHS for f1, f2 in FLANKS for d in (True, False)]
    stripes = [_gap_pair(rng, f1, L, 64, d) for L in GAP_LENGTHS for f1 in STRIPE_STARTS for d in (True, False)]
    clipped = [_gap_pair(rng, f1, L, f2, d, int(rng.integers(5, 31)), int(rng.integers(5, 31)))
               for L in GAP_LENGTHS for f1, f2 in FLANKS for d in (True, False)]
    return [("flanks", S.from_pairs(flanks)), ("stripes", S.from_pairs(stripes)),
            ("clipped", S.from_pairs(clipped)),
            ("region415", _shared_ref_batch(_gap_region(rng, 415, 16))),
            ("region900", _shared_ref_batch(_gap_region(rng, 900, 16)))]


REGION_SETS = ("region415", "region900")


# ---- the boundary of the fast variant's proof -----------------------------
def _tailed(x, n, tail):
    return x * (n - len(tail)) + tail


def boundary_pairs(seed=203):
    rng = np.random.default_rng(seed)
    t = _rand(rng, 20).tobytes()
    t1 = _rand(rng, 20).tobytes()
    A, C = b"A", b"C"
    pairs = [
        (_tailed(A, 1023, t), _tailed(C, 1023, t)),     # 0: the measured pair
        (_tailed(A, 1023, t), _tailed(C, 1024, t)),     # 1
        (_tailed(C, 1023, t), _tailed(A, 1023, t)),     # 2: pair 0 transposed
        (_tailed(C, 1022, t), _tailed(A, 1024, t)),
        (t1 + _tailed(A, 1003, t), t1 + _tailed(C, 1002, t)),   # 4: a forced interior gap next to the cutoff
    ]
    for n1, n2 in ((64, 64), (65, 65), (200, 200), (415, 415), (65, 200), (200, 64)):
        pairs.append((_tailed(A, n1, t), _tailed(C, n2, t)))
    return pairs


BOUNDARY_MEASURED = 0      # index of the A.../C... 1023 x 1023 pair in boundary_pairs()
BOUNDARY_INTERIOR_GAP = 4


def boundary_cases(seed=203):
    """[dict(name, params, strategies, fast, binds, pairs, batch)]: `fast` is the
    side of fast_ok the row claims for the batch's maxima (1023 x 1024), `binds`
    whether the cutoff is claimed to bind on the measured pair."""
    pairs = boundary_pairs(seed)
    b = S.from_pairs(pairs)
    rows = [
        ("indel_in", (1000, -47000, -50000000, -1000), (S.INDEL, S.LEADING_INDEL), True, False),
        ("indel_out", (1000, -48000, -50000000, -1000), (S.INDEL, S.LEADING_INDEL), False, False),
        ("clip_in", (1000, -97000, -50000000, -100000), (S.SOFTCLIP, S.IGNORE), True, False),
        ("clip_out", (1000, -98000, -50000000, -100000), (S.SOFTCLIP, S.IGNORE), False, False),
        ("indel_binds", (1000, -97000, -50000000, -100000), (S.INDEL,), False, True),
        ("cutoff_clause_only", (1000, -99000, -1000000, -1000), (S.INDEL,), False, False),
        # outside by the cutoff clause alone (v is about 2.0e8 < 2^28), and the cutoff binds
        ("binds_by_clause_only", (1000, -97000, -50000000, -1000), (S.INDEL, S.LEADING_INDEL), False, True),
    ]
    return [dict(name=n, params=p, strategies=st, fast=f, binds=bd, pairs=pairs, batch=b)
            for n, p, st, f, bd in rows]


# ---- order ----------------------------------------------------------------
def order_cases(seed=204):
    """Three small batches whose last stripes are short (n1 % 64 small, so the
    DP stops the stripe early and writes no backtrack words past its rows)."""
    rng = np.random.default_rng(seed)
    out = []
    for name, n1s, n2s in (("short_stripes", (65, 66, 67, 129, 130, 193, 1, 2), (300, 9, 64, 200, 8, 129, 40, 1)),
                           ("tiny", (1, 2, 3, 65, 66, 5), (1, 1, 2, 1, 3, 900)),
                           ("gaps", (66, 130, 194, 258, 67), (200, 60, 130, 400, 7))):
        pairs = []
        for n1, n2 in zip(n1s, n2s):
            r = S._window(rng, n1)
            if n2 > n1:   # the alt is the window with an insertion
                p = int(rng.integers(0, n1 + 1))
                a = np.concatenate([r[:p], _rand(rng, n2 - n1), r[p:]])
            else:         # ... with a deletion
                p = int(rng.integers(0, n2 + 1))
                a = np.concatenate([r[:p], r[p + n1 - n2:]])
            a = S._mutate(rng, a, 0.02, 0.0, 0.0) if n2 > 8 else a
            pairs.append((r.tobytes(), a.tobytes()))
        out.append((name, S.from_pairs(pairs)))
    return out


# ---- what the golden file was made from -----------------------------------
def batch_hash(b) -> str:
    h = hashlib.sha256()
    for k in ("ref_off", "ref_len", "refs", "alt_off", "alt_len", "alts"):
        h.update(k.encode())
        h.update(np.ascontiguousarray(b[k]).tobytes())
    return h.hexdigest()


def golden_plan():
    """[(case name, batch, params, strategy)]: every run whose reference answer
    tests/golden/sw_cases_golden.npz holds (shortcut on)."""
    plan = []
    union, _ = layout_union()
    for p in (S.NEW_SW_PARAMETERS, S.ORIGINAL_DEFAULT):
        for st in S.STRATEGIES:
            plan.append((f"layout_{'_'.join(map(str, p))}_{st}", union, p, st))
    for name, b in gap_pairs():
        for p in S.PARAM_SETS:
            for st in S.STRATEGIES:
                plan.append((f"{name}_{'_'.join(map(str, p))}_{st}", b, p, st))
    for row in boundary_cases():
        for st in row["strategies"]:
            plan.append((f"boundary_{row['name']}_{st}", row["batch"], row["params"], st))
    for name, b in order_cases():
        plan.append((f"order_{name}", b, S.NEW_SW_PARAMETERS, S.SOFTCLIP))
    return plan


def inputs_hash() -> str:
    h = hashlib.sha256()
    for name, b, p, st in golden_plan():
        h.update(f"{name}|{p}|{st}|{batch_hash(b)}\n".encode())
    return h.hexdigest()


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_cases_golden.npz")


def load_golden(path=GOLDEN):
    """tests/golden/make_sw_cases_golden.py: case name -> (offsets, CIGARs) of
    the reference aligner, and the hash of the inputs they were made from."""
    g = np.load(path, allow_pickle=False)
    text = lambda k: g[k].tobytes().decode()   # noqa: E731
    cases = {name: (g[name + "_offset"], text(name + "_cigar").split("\n")) for name in text("cases").split("\n")}
    return dict(cases=cases, inputs_sha256=text("inputs_sha256"))
