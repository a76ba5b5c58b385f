"""CPU: the Smith-Waterman oracle against the reference on the case families
of sw_cases.py, none of which sw_golden.npz holds.

tests/golden/sw_cases_golden.npz has the reference aligner's offsets and
CIGARs for every run of sw_cases.golden_plan() (make_sw_cases_golden.py), made
from inputs whose hash it records. The oracle must reproduce all of them, and
its end-point score must equal the row-wise int64 DP of sw_census.dp, which
shares no code with it.
"""
import numpy as np
import pytest

import sw_cases as K
import sw_census as Z
import sw_workloads as S


@pytest.fixture(scope="module")
def golden():
    return K.load_golden()


def test_golden_was_made_from_these_inputs(golden):
    assert golden["inputs_sha256"] == K.inputs_hash()
    assert list(golden["cases"]) == [name for name, _, _, _ in K.golden_plan()]


def test_golden_covers_every_family_strategy_and_param_set(golden):
    names = set(golden["cases"])
    tag = lambda p: "_".join(map(str, p))   # noqa: E731
    for st in S.STRATEGIES:
        for p in (S.NEW_SW_PARAMETERS, S.ORIGINAL_DEFAULT):
            assert f"layout_{tag(p)}_{st}" in names
        for name, _ in K.gap_pairs():
            for p in S.PARAM_SETS:
                assert f"{name}_{tag(p)}_{st}" in names
    for row in K.boundary_cases():
        for st in row["strategies"]:
            assert f"boundary_{row['name']}_{st}" in names


def test_oracle_reproduces_the_reference(golden, sw_oracle_lib):
    for name, b, p, st in K.golden_plan():
        off, cig = sw_oracle_lib.batch(b, p, st, shortcut=True, nthreads=4)
        g_off, g_cig = golden["cases"][name]
        assert len(g_cig) == len(cig) == len(b["ref_len"]), name
        bad = [k for k in range(len(cig)) if cig[k] != g_cig[k] or off[k] != g_off[k]]
        assert not bad, (name, len(bad), [(k, cig[k], g_cig[k], off[k], g_off[k]) for k in bad[:3]])


def test_census_dp_score_equals_the_oracle_score(sw_oracle_lib):
    """The best end-point score, from two implementations: hco_sw_align's
    *score and the int64 row sweep. On the boundary family the sweep also runs
    with no cutoff; there its lowest H says how close the pair comes."""
    runs = []
    for row in K.boundary_cases():
        for st in row["strategies"]:
            runs += [(row["params"], st, row["pairs"][k]) for k in (0, 1, 4, 5, 6, 9, 10)]
    union, _ = K.layout_union()
    for k in (0, 5, 12, 21, 33, 42, 47, 54, 62):
        runs += [(p, st, S.pair(union, k)) for p in (S.NEW_SW_PARAMETERS, S.ORIGINAL_DEFAULT) for st in S.STRATEGIES]
    gaps = dict(K.gap_pairs())
    for name, ks in (("clipped", (0, 1, 46, 47)), ("stripes", (90, 91)), ("region415", (3,))):
        runs += [(S.NEW_SW_PARAMETERS, st, S.pair(gaps[name], k)) for k in ks for st in (S.SOFTCLIP, S.INDEL)]
    for p, st, (r, a) in runs:
        d = Z.dp(p, st, r, a)
        assert d["score"] == sw_oracle_lib.score(r, a, p, st), (p, st, len(r), len(a))
        assert d["n_best"] >= 1


def test_oracle_scores_are_zero_for_shortcut_pairs(sw_oracle_lib):
    r = b"ACGTTGCA" * 200   # 1600 bases: past the aligner's limit, the shortcut still answers
    b = S.from_pairs([(r, r), (r[:100], r[:100]), (r[:100], r[:90])])
    sc = sw_oracle_lib.scores(b)
    assert sc[0] == 0 and sc[1] == 0 and sc[2] == 90 * 200
    assert sw_oracle_lib.scores(b, shortcut=False)[1] == 100 * 200
