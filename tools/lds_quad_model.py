#!/usr/bin/env python3
"""LDS cycles per read of the prior tables, by Monte-Carlo on the CPU.

A wave64 ds_read_b64 is served in two groups of 32 lanes, one LDS cycle per
group when conflict-free; the bank of byte address a is (a / 4) mod 64, lanes
with the same address share a cycle (broadcast), and every further distinct
address on a busy bank adds one (MI355X LDS banking). So a group costs the
maximum over the banks of the number of distinct addresses on it, and a read
the sum over its groups. A ds_read_b128 is served in four groups of 16 lanes
that are not contiguous (B128_GROUPS), same banks, four banks per address.

Lanes are independent: quality q uniform in [qlo, qhi] (S2: 43..73) and each
match bit set with probability p (0.25: a row of a read against a random hap).

    pair table   a = 32 q + 8 (2 bits)                      (seg_common.hpp ptab)
    quad table   a = 128 r + 8 c,  r = q - qlo,  c = 4 bits, region B at +5120
                 (a multiple of 256: the same banks), plain or with the swizzle
                 c = bits ^ ((r >> 1) & 15)                 (round 11's form)
    b128 table   a = 256 r + 16 c, one 16-byte read per four columns, plain or
                 with c = bits ^ (r & 15)                   (fill_qtab, quad_row)

    shared table a = 256 (q & 63) + 16 (bits ^ (q & 15)), the workgroup's 64 rows by
                 absolute quality                           (fill_shared_tabs, quad_base2)
    window byte  a = 1024 code + 256 (g / 4) + 4 lane + g % 4, the spread window's
                 ds_read_u8 of group g                      (seg_spread.hpp)

    python tools/lds_quad_model.py [--json OUT] [--json128 OUT128] [--json-byte OUTB]

--json writes the ds_read_b64 layouts (per read), --json128 the comparison per
four columns: two ds_read_b64 of the swizzled quad table against one
ds_read_b128, with the spread of each over SEEDS further seeds. --json-byte
writes the byte form's: the ds_read_b128 of the shared 64-row table and the
ds_read_u8 of the spread window, one of each per four columns.

A read of four bytes or fewer is served in one group of all 64 lanes, and lanes
in the same dword share it: the byte read is conflict-free by layout, since the
lanes of one group's read sit in 64 consecutive dwords whatever their codes
(byte_read_cycles checks it for every group over random codes).
"""
import json
import sys

import numpy as np

B64_GROUPS = [list(range(0, 32)), list(range(32, 64))]
B128_GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]
B32_GROUPS = [list(range(64))]
SEEDS = 8   # further seeds for the seed-to-seed spread (fewer draws each)


def cycles(addr, groups=B64_GROUPS, width=8):
    """Mean LDS cycles per wave read. addr: (n, 64) byte addresses of `width`-byte
    reads, width-aligned, so an entry's first bank names its whole set of banks."""
    n = addr.shape[0]
    tot = 0
    for lanes in groups:
        worst = np.zeros(n, np.int64)
        a = np.sort(addr[:, lanes], axis=1)
        first = np.ones_like(a, bool)
        first[:, 1:] = a[:, 1:] != a[:, :-1]          # one per distinct address
        bank = (a // 4) % 64                          # the entry's first bank (a is width-aligned)
        for b in range(0, 64, width // 4):
            worst = np.maximum(worst, ((bank == b) & first).sum(axis=1))
        tot += worst.sum()
    return tot / n


def draw(rng, n, qlo, qhi, p):
    q = rng.integers(qlo, qhi + 1, (n, 64))
    bits = (rng.random((n, 64, 4)) < p).astype(np.int64)
    pat2 = bits[:, :, 0] * 2 + bits[:, :, 1]
    pat4 = pat2 * 4 + bits[:, :, 2] * 2 + bits[:, :, 3]
    return q, pat2, pat4, q - qlo


def per_four_columns(r, pat4):
    """LDS-array cycles per four columns of a row: (two ds_read_b64 of the swizzled
    quad table, ds_read_b128 swizzled, ds_read_b128 plain)."""
    return (2 * cycles(128 * r + 8 * (pat4 ^ ((r >> 1) & 15))),
            cycles(256 * r + 16 * (pat4 ^ (r & 15)), B128_GROUPS, 16),
            cycles(256 * r + 16 * pat4, B128_GROUPS, 16))


def shared_table_addr(q, pat4):
    """The workgroup's quad table: row q & 63, column pattern ^ (q & 15)."""
    return 256 * (q & 63) + 16 * (pat4 ^ (q & 15))


def window_byte_addr(code, g, lane=None):
    """Byte address of group g of (code, lane) in a wave's spread window."""
    lane = np.arange(64) if lane is None else lane
    return 1024 * code + 256 * (g // 4) + 4 * lane + g % 4


def byte_read_cycles(rng, n=2000):
    """LDS cycles of the ds_read_u8 of each of the 16 groups, lanes on random read
    codes: [1.0] * 16 when the layout is conflict-free."""
    out = []
    for g in range(16):
        a = window_byte_addr(rng.integers(0, 5, (n, 64)), g)
        out.append(float(cycles(a // 4 * 4, B32_GROUPS, 4)))
    return out


def main():
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    out128 = sys.argv[sys.argv.index("--json128") + 1] if "--json128" in sys.argv else None
    rng = np.random.default_rng(7)
    n, qlo, qhi, p = 20000, 43, 73, 0.25
    q, pat2, pat4, r = draw(rng, n, qlo, qhi, p)
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
    # Per four columns, and how far each figure moves from seed to seed.
    main4 = per_four_columns(r, pat4)
    seeds = np.array([per_four_columns(*draw(np.random.default_rng(100 + s), n // 4, qlo, qhi, p)[:1:-1])
                      for s in range(SEEDS)])
    names = ["two ds_read_b64, 128-byte rows, column ^ ((r >> 1) & 15)",
             "ds_read_b128, 256-byte rows, column ^ (r & 15)",
             "ds_read_b128, 256-byte rows, plain"]
    rows128 = []
    for i, name in enumerate(names):
        x = dict(layout=name, lds_cycles_per_four_columns=round(float(main4[i]), 2),
                 conflict_free=4, lds_instructions_per_four_columns=2 if i == 0 else 1,
                 seed_to_seed=dict(seeds=SEEDS, draws=n // 4, min=round(float(seeds[:, i].min()), 3),
                                   max=round(float(seeds[:, i].max()), 3), std=round(float(seeds[:, i].std()), 3)),
                 lanes="independent", q=[qlo, qhi], p_match=p, draws=n)
        if i == 0:
            x["lds_cycles_per_read"] = round(float(main4[0]) / 2, 2)
        rows128.append(x)
        print(json.dumps(x))
    outb = sys.argv[sys.argv.index("--json-byte") + 1] if "--json-byte" in sys.argv else None
    shared = cycles(shared_table_addr(q, pat4), B128_GROUPS, 16)
    bytes_ = byte_read_cycles(np.random.default_rng(11))
    rowsb = [dict(layout="ds_read_b128, 64 rows of 256 bytes by q & 63, column ^ (q & 15)",
                  lds_cycles_per_four_columns=round(float(shared), 2), conflict_free=4,
                  lanes="independent", q=[qlo, qhi], p_match=p, draws=n),
             dict(layout="ds_read_u8, spread window [code][g / 4][lane][g % 4]",
                  lds_cycles_per_four_columns=round(max(bytes_), 2), conflict_free=1, groups=16,
                  lanes="random read codes", draws=2000)]
    for x in rowsb:
        print(json.dumps(x))
    for path, rr in ((out, rows), (out128, rows128), (outb, rowsb)):
        if path:
            with open(path, "w") as f:
                for x in rr:
                    f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
