"""CPU, on the expected side only (no engine): what the Smith-Waterman case
families of sw_cases.py exercise, stated by sw_census.py and asserted here, and
that the inputs the aligner's tests had before (the edge grid, W1, W2 of 24
regions, W3 of 4 regions, the heavy-indel batch) lack each property. Expected
CIGARs of the new families are the reference's (sw_cases_golden.npz); those of
the old inputs come from the oracle, which sw_golden.npz pins to the reference
on them."""
import pytest

import sw_cases as K
import sw_census as Z
import sw_workloads as S

NEW = "_".join(map(str, S.NEW_SW_PARAMETERS))


@pytest.fixture(scope="module")
def golden():
    return K.load_golden()["cases"]


def old_inputs():
    return [("edge", S.from_pairs(S.edge_pairs())), ("edge5", S.from_pairs(S.edge_pairs(seed=5))),
            ("W1", S.config("W1")), ("W2_24", S.config("W2", 24)), ("W3_4", S.config("W3", 4)),
            ("heavy", S.regions(8, 64, (200, 900), seed=77, snp=0.05, indel=0.02, trim=0.6))]


def test_layout_batches_take_the_tall_layout_and_old_inputs_never_do():
    batches = K.layout_batches()
    assert [Z.maxima(b) for _, b in batches] == list(K.LAYOUT_MAXIMA)
    tall = [name for name, b in batches if Z.tall_layout(*Z.maxima(b))]
    assert tall == ["1023x1", "1023x8", "1023x9", "600x64"]
    for name, b in batches:
        n1max, n2max = Z.maxima(b)
        # the second branch of fslots sizes rowF exactly when the layout is tall
        assert (Z.fslots(n1max, n2max) != Z.row_slots(n2max)) == (name in tall)
        assert Z.fslots(n1max, n2max) >= n1max + 1
    for name, b in old_inputs():
        assert not Z.tall_layout(*Z.maxima(b)), name


def test_layout_batches_sizes_and_partly_filled_workgroups():
    union, where = K.layout_union()
    assert Z.maxima(union) == (1023, 1024)
    assert sorted(k for ks in where.values() for k in ks) == list(range(len(union["ref_len"])))
    r1, r2 = set(), set()
    for (name, b), (N1, N2) in zip(K.layout_batches(), K.LAYOUT_MAXIMA):
        n = len(b["ref_len"])
        assert n in K.LAYOUT_COUNTS and n % 2 == 1 and n % 4 != 0      # a last workgroup with idle waves at 2 and 4
        assert (b["ref_len"][0], b["alt_len"][0]) == (N1, N2)          # the maximal pair
        assert [S.pair(b, k) for k in range(n)] == [S.pair(union, k) for k in where[name]]
        r1 |= {int(x) % 64 for x in b["ref_len"]}
        r2 |= {int(x) % 8 for x in b["alt_len"]}
        if N1 >= 64:
            assert {int(x) % 64 for x in b["ref_len"]} & {0, 1, 63}
    assert {0, 1, 63} <= r1 and {0, 1, 7} <= r2
    # n2max of 1, 8, 9, 64 and 200: no old batch had a row buffer for fewer than 400 columns
    assert min(Z.maxima(b)[1] for _, b in old_inputs()) >= 400


def test_long_interior_gaps_under_the_production_strategy(golden, sw_oracle_lib):
    for st in (S.SOFTCLIP, S.IGNORE):
        new = {name: Z.batch_census(golden[f"{name}_{NEW}_{st}"][1]) for name, _ in K.gap_pairs()}
        assert max(c["interior_i"] for c in new.values()) >= 129
        assert max(c["interior_d"] for c in new.values()) >= 129
        assert new["flanks"]["interior_i"] == new["flanks"]["interior_d"] == 500
        for name in ("flanks", "stripes", "clipped"):
            assert new[name]["interior_i"] >= 129 and new[name]["interior_d"] >= 129, name
        for name in K.REGION_SETS:
            assert max(new[name]["interior_i"], new[name]["interior_d"]) >= 64, name
        assert new["clipped"]["clip_next_to_long_gap"] >= 2
        if st == S.SOFTCLIP:
            assert new["clipped"]["lead_s"] >= 5 and new["clipped"]["trail_s"] >= 5
        worst_i = worst_d = 0
        for name, b in old_inputs():
            c = Z.batch_census(sw_oracle_lib.batch(b, S.NEW_SW_PARAMETERS, st, nthreads=8)[1])
            worst_i, worst_d = max(worst_i, c["interior_i"]), max(worst_d, c["interior_d"])
            assert c["clip_next_to_long_gap"] == 0, name
        print(f"strategy {st}: old inputs' longest interior I {worst_i}, D {worst_d}")
        assert worst_i < 64 and worst_d < 64


def test_gaps_start_next_to_the_stripe_borders(golden):
    """The stripes set opens its gap after 60..70 and 120..135 matched bases:
    the run of a deletion then crosses rows 64 / 128, that of an insertion
    columns 64 / 128."""
    _, cig = golden[f"stripes_{NEW}_{S.SOFTCLIP}"]
    starts = {}
    for c in cig:
        el = Z.elements(c)
        if len(el) == 3 and el[0][1] == el[2][1] == "M" and el[1][1] in "ID" and el[1][0] >= 63:
            starts.setdefault(el[1][1], set()).add(el[0][0])
    for op in "ID":
        assert {x for x in starts[op] if 60 <= x <= 70} and {x for x in starts[op] if 120 <= x <= 135}
        assert starts[op] & {63, 64, 65} and starts[op] & {127, 128, 129}


def test_boundary_rows_lie_on_the_side_they_claim():
    rows = K.boundary_cases()
    assert {r["fast"] for r in rows} == {True, False}
    for r in rows:
        n1max, n2max = Z.maxima(r["batch"])
        assert (n1max, n2max) == (1023, 1024)
        for st in r["strategies"]:
            assert Z.fast_ok(r["params"], st, n1max, n2max) == r["fast"], (r["name"], st)
    for name in ("cutoff_clause_only", "binds_by_clause_only"):
        only = next(r for r in rows if r["name"] == name)
        assert all(Z.fast_ok_without_cutoff_clause(only["params"], st, 1023, 1024) for st in only["strategies"])
    # ... while the other binding row is refused twice over
    assert not Z.fast_ok_without_cutoff_clause(rows[4]["params"], S.INDEL, 1023, 1024) and rows[4]["binds"]
    # the reference's own parameter sets and CUTOFF_PARAMS are far from the boundary
    for p in S.PARAM_SETS:
        assert Z.fast_ok(p, S.INDEL, 1023, 1024) and Z.fast_ok(tuple(20 * x for x in p), S.INDEL, 1023, 1024)
    assert not Z.fast_ok(tuple(x // 4 for x in S.CUTOFF_PARAMS), S.INDEL, 1023, 1024)


def test_boundary_rows_reach_the_cutoff(golden):
    binds = []
    for r in rows_with_dp():
        d = r["dp"]
        if r["fast"]:     # just inside: H next to the cutoff, and the cutoff inert
            assert d["lowest_h"] <= -95000000 and d["lowest_h"] >= Z.MIN_CUTOFF and not d["bound"], r["name"]
        assert d["bound"] == r["binds"], r["name"]
        if d["bound"]:
            assert d["lowest_h"] < Z.MIN_CUTOFF and d["lowest_h_cut"] >= Z.MIN_CUTOFF
            binds.append(r["name"])
    assert binds and all(not r["fast"] for r in rows_with_dp() if r["name"] in binds)
    # A just-outside row that does not bind still runs within 2 % of the cutoff.
    assert all(r["dp"]["lowest_h"] <= -98000000 for r in rows_with_dp() if r["name"] in ("indel_out", "clip_out"))
    # The pair with the forced gap: an interior deletion on a path next to the cutoff.
    for name in ("indel_in", "indel_out"):
        row = next(r for r in K.boundary_cases() if r["name"] == name)
        c = Z.cigar_census(golden[f"boundary_{name}_{S.INDEL}"][1][K.BOUNDARY_INTERIOR_GAP])
        assert c["interior_d"] >= 1
        ref, alt = row["pairs"][K.BOUNDARY_INTERIOR_GAP]
        d = Z.dp(row["params"], S.INDEL, ref, alt)
        assert -100000000 <= d["lowest_h"] <= -95000000 and not d["bound"]
        assert int(d["last_col"][len(ref)]) <= -95000000     # H(n1, n2): the traced path's own score


_ROWS = []


def rows_with_dp():
    """Every boundary row with sw_census.dp of the measured pair (once)."""
    if not _ROWS:
        for r in K.boundary_cases():
            ref, alt = r["pairs"][K.BOUNDARY_MEASURED]
            assert (len(ref), len(alt)) == (1023, 1023)
            _ROWS.append(dict(r, dp=Z.dp(r["params"], r["strategies"][0], ref, alt)))
    return _ROWS


def test_order_cases_have_short_last_stripes():
    for name, b in K.order_cases():
        short = [Z.short_last_stripe(int(n1), int(n2)) for n1, n2 in zip(b["ref_len"], b["alt_len"])]
        assert sum(short) >= 3, name
        assert Z.maxima(b)[0] < 300
