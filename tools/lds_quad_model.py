#!/usr/bin/env python3
"""LDS cycles per ds_read_b64 of the prior tables, by Monte-Carlo on the CPU.

A wave64 ds_read_b64 is served in two groups of 32 lanes, one LDS cycle per
group when conflict-free; the bank of byte address a is (a / 4) mod 64, lanes
with the same address share a cycle (broadcast), and every further distinct
address on a busy bank adds one (MI355X LDS banking). So a group costs the
maximum over the banks of the number of distinct addresses on it, and a read
the sum over its two groups.

Lanes are independent: quality q uniform in [qlo, qhi] (S2: 43..73) and each
match bit set with probability p (0.25: a row of a read against a random hap).

    pair table   a = 32 q + 8 (2 bits)                      (seg_common.hpp ptab)
    quad table   a = 128 r + 8 c,  r = q - qlo,  c = 4 bits, region B at +5120
                 (a multiple of 256: the same banks), plain or with the swizzle
                 c = bits ^ ((r >> 1) & 15)                 (fill_qtab, quad_row)

    python tools/lds_quad_model.py [--json OUT]
"""
import json
import sys

import numpy as np


def cycles(addr):
    """Mean LDS cycles per wave read. addr: (n, 64) byte addresses of 8-byte reads."""
    n = addr.shape[0]
    tot = 0
    for g in (addr[:, :32], addr[:, 32:]):
        worst = np.zeros(n, np.int64)
        a = np.sort(g, axis=1)
        first = np.ones_like(a, bool)
        first[:, 1:] = a[:, 1:] != a[:, :-1]          # one per distinct address
        bank = (a // 4) % 64                          # an 8-byte entry: banks bank, bank + 1 (a is 8-aligned)
        for b in range(0, 64, 2):
            worst = np.maximum(worst, ((bank == b) & first).sum(axis=1))
        tot += worst.sum()
    return tot / n


def main():
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    rng = np.random.default_rng(7)
    n, qlo, qhi, p = 20000, 43, 73, 0.25
    q = rng.integers(qlo, qhi + 1, (n, 64))
    bits = (rng.random((n, 64, 4)) < p).astype(np.int64)
    pat2 = bits[:, :, 0] * 2 + bits[:, :, 1]
    pat4 = pat2 * 4 + bits[:, :, 2] * 2 + bits[:, :, 3]
    r = q - qlo
    rows = [
        dict(layout="pair table, 32-byte rows", lds_cycles_per_read=cycles(32 * q + 8 * pat2)),
        dict(layout="quad table, 128-byte rows, plain", lds_cycles_per_read=cycles(128 * r + 8 * pat4)),
        dict(layout="quad table, 128-byte rows, column ^ ((r >> 1) & 15)",
             lds_cycles_per_read=cycles(128 * r + 8 * (pat4 ^ ((r >> 1) & 15)))),
    ]
    for x in rows:
        x.update(lds_cycles_per_read=round(float(x["lds_cycles_per_read"]), 2),
                 conflict_cycles_per_read=round(float(x["lds_cycles_per_read"]) - 2, 2),
                 lanes="independent", q=[qlo, qhi], p_match=p, draws=n)
        print(json.dumps(x))
    if out:
        with open(out, "w") as f:
            for x in rows:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
