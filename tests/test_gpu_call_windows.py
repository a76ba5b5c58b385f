"""GPU: hc_call_windows (include/hc_call.h) against the chain it replaces: the
restatement's prepared reads (prep_restate.py) through hcasm.assemble, the two
skip rules of call_region and hcregion.call_regions. Window statuses, haplotype
bytes and score bits, begins and CIGARs, every site field, the surviving read
indices and the matrices bit for bit; batched and one by one.

The seed is call_cases.SEED = 20261019: with it the expected side has at least
12 of 24 windows with an emitted site and each early ending at least once
(test_the_set_reaches_every_ending checks exactly that, on the expected side)."""
import numpy as np
import pytest

import call_cases as CC
import hccall
import hcprep
import prep_restate as PR
from gt_restate import EMITTED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wins():
    return CC.windows()


@pytest.fixture(scope="module")
def exp(engine, wins):
    return CC.expected(wins)


@pytest.fixture(scope="module")
def got(engine, wins):
    return hccall.call_windows(wins, want_L=True, want_site_reads=True, want_cigars=True)


def test_the_set_reaches_every_ending(wins, exp):
    """On the expected side, so that it cannot hide a failure."""
    assert len(wins) == 24
    emitted = {s["region"] for s in exp["sites"] if s["status"] == EMITTED}
    assert len(emitted) >= 12, sorted(emitted)
    status = [w["status"] for w in exp["windows"]]
    assert status[2] == CC.NO_READS and not wins[2]["reads"]                      # no reads at all
    assert status[3] == CC.NO_READS and wins[3]["reads"]                          # every read filtered
    assert set(exp["windows"][3]["reasons"]) <= {PR.MAPQ, PR.DUPLICATE, PR.SECONDARY, PR.MATE_CONTIG}
    assert status[4] == CC.NO_VARIATION and len(exp["windows"][4]["haps"]) == 1   # no variant
    reasons = {c for w in exp["windows"] for c in w["reasons"]}
    assert reasons == {PR.KEPT, PR.MAPQ, PR.DUPLICATE, PR.SECONDARY, PR.MATE_CONTIG, PR.MIN_LENGTH}
    assert any("D" in r["cigar"] for r in wins[1]["reads"])
    assert any("S" in r["cigar"] and r["flag"] & 0x10 for w in wins for r in w["reads"])
    assert any("S" in r["cigar"] and not r["flag"] & 0x10 for w in wins for r in w["reads"])


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


def _same_site(a, b):
    for k in ("region", "status", "begin", "loc_end", "n_alleles", "alleles", "n_keep", "keep_is_null", "genotype_index",
              "a1", "a2", "genotype_quality"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["hap_allele"].tolist() == b["hap_allele"].tolist() and a["keep"].tolist() == b["keep"].tolist()
    assert _bits(a["genotype_likelihoods"]) == _bits(b["genotype_likelihoods"])


def _assert_equal(got, exp, tag):
    assert len(got["windows"]) == len(exp["windows"])
    for k, (g, e) in enumerate(zip(got["windows"], exp["windows"])):
        at = (tag, k)
        assert (g["status"], g["asm_status"], g["kmer_size"]) == (e["status"], e["asm_status"], e["kmer_size"]), at
        assert [h[0] for h in g["haps"]] == [h[0] for h in e["haps"]], at
        assert _bits([h[1] for h in g["haps"]]) == _bits([h[1] for h in e["haps"]]), at
        assert g["reads"] == e["reads"], at
        assert [r["drop_reason"] for r in g["prep"]["records"]] == e["reasons"], at
        if e["status"] == CC.CALLED:
            assert g["alignments"] == e["alignments"], at
            assert g["L"].shape == e["L"].shape and _bits(g["L"]) == _bits(e["L"]), at
        else:
            assert all(a == (-1, None) for a in g["alignments"]) and g["L"].shape == (0, len(e["haps"])), at
    assert len(got["sites"]) == len(exp["sites"]), tag
    for a, b in zip(got["sites"], exp["sites"]):
        _same_site(a, b)


def test_batched_equals_the_chain(got, exp):
    _assert_equal(got, exp, "batched")


def test_prep_records_equal_the_restatement(got, wins):
    for k, (g, w) in enumerate(zip(got["windows"], wins)):
        e = PR.records(CC.prep_window(w))
        assert all(PR.same_record(a, b) for a, b in zip(g["prep"]["records"], e["records"])), k
        assert (g["prep"]["kept"], g["prep"]["n_kept"], g["prep"]["kept_bases"]) == (e["kept"], e["n_kept"], e["kept_bases"])
    assert hcprep.prep_reads([CC.prep_window(w) for w in wins]) == [g["prep"] for g in got["windows"]]


def test_one_by_one_equals_the_chain(engine, wins, exp):
    for k, w in enumerate(wins):
        one = hccall.call_windows([w], want_L=True, want_site_reads=True, want_cigars=True)
        e = dict(windows=[exp["windows"][k]], sites=[dict(s, region=0) for s in exp["sites"] if s["region"] == k])
        _assert_equal(one, e, f"window {k} alone")


def test_flags_and_accessor_errors(engine, wins):
    plain = hccall.call_windows(wins[:2])
    assert all(s["keep_is_null"] for s in plain["sites"]) and "L" not in plain["windows"][0]
    import ctypes as C
    p = hccall.Prepared(wins[:1])
    h = p.run(0)
    try:
        L = hccall.lib()
        assert L.hc_call_result_matrix(h, 0, None, None, None) == -1
        b, c = C.c_int32(), C.c_char_p()
        assert L.hc_call_result_hap(h, 0, 0, None, None, None, C.byref(b), C.byref(c)) == -1
        assert L.hc_call_result_window(h, 1, None, None, None, None) == -1
    finally:
        p.free(h)
    f64 = hccall.call_windows(wins[:1], use_double=True)
    assert [s["begin"] for s in f64["sites"]] == [s["begin"] for s in plain["sites"] if s["region"] == 0]
