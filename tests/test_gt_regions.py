"""Genotyper drop-in (hc_gt_call_regions): events, alleles, haplotype -> allele
maps and kept reads on the device, ahead of the existing arithmetic.

CPU: the Python restatement (tests/gt_restate.py) is pinned by hand-derived
cases written out literally; the seeded random set covers every outcome; the
library exports the new symbols and has no CPU path. GPU (-m gpu): every field
of every site record equals the restatement, likelihoods as bits."""
import copy
import subprocess

import numpy as np
import pytest

import gt_restate as RS
import gt_workloads as G

REF = b"ACGTACGTAC"   # window positions 0..9, contig coordinates 100..109
PB = 100


def region(haps, ref=REF, pb=PB, origin=None, reads=((90, 120),), seed=0):
    """haps: (bases, begin, cigar) after the reference path."""
    hl = [dict(bases=ref, begin=0, cigar=f"{len(ref)}M")] + [dict(bases=b, begin=s, cigar=c) for b, s, c in haps]
    ob, oe = origin or (pb, pb + len(ref))
    rng = np.random.default_rng(seed)
    return dict(ref=ref, padded_begin=pb, origin_begin=ob, origin_end=oe, haps=hl,
                read_begin=np.array([r[0] for r in reads], np.int64), read_end=np.array([r[1] for r in reads], np.int64),
                L=np.ascontiguousarray(rng.uniform(-4.0, 0.0, (len(reads), len(hl)))))


def site(begin, loc_end, alleles, hap_allele, keep=(0,)):
    return dict(begin=begin, loc_end=loc_end, alleles=list(alleles), hap_allele=list(hap_allele), keep=list(keep))


SKIPPED = "skipped"
EIGHT = [(b"ACGTCCGTAC", 0, "10M"), (b"ACGTGCGTAC", 0, "10M"), (b"ACGTTCGTAC", 0, "10M"),
         (b"ACGTAACGTAC", 0, "5M1I5M"), (b"ACGTACCGTAC", 0, "5M1I5M"), (b"ACGTAGCGTAC", 0, "5M1I5M"),
         (b"ACGTATCGTAC", 0, "5M1I5M")]

# name -> (region, expected sites). Window ACGTACGTAC at 100: position 4 is 'A' (104), 6 is 'G', 7 is 'T'.
HAND = {
    # reads: [begin-2, loc_end+2) = [102, 107) is overlapped by [90,103) and [106,120), not by [90,102) or [107,120)
    "snp_het": (region([(b"ACGTTCGTAC", 0, "10M")], reads=((90, 103), (90, 102), (106, 120), (107, 120))),
                [site(104, 105, [b"A", b"T"], [0, 1], keep=[0, 2])]),
    "insertion": (region([(b"ACGTAGGCGTAC", 0, "5M2I5M")]), [site(104, 105, [b"A", b"AGG"], [0, 1])]),
    "deletion": (region([(b"ACGTAAC", 0, "5M3D2M")]), [site(104, 108, [b"ACGT", b"A"], [0, 1])]),
    "deletion_spans_snp": (region([(b"ACGTAAC", 0, "5M3D2M"), (b"ACGTACTTAC", 0, "10M")]),
                           [site(104, 108, [b"ACGT", b"A"], [0, 1, 0]),
                            site(106, 107, [b"G", b"*", b"T"], [0, 1, 2])]),
    "snp_suppresses_insertion": (region([(b"ACGTTGGCGTAC", 0, "5M2I5M")]), [site(104, 105, [b"A", b"T"], [0, 1])]),
    "ins_then_del": (region([(b"ACGTAGGAC", 0, "5M2I3D2M")]), [site(104, 105, [b"A", b"AGG"], [0, 1])]),
    "del_then_ins": (region([(b"ACGTAGGAC", 0, "5M3D2I2M")]),
                     [site(104, 108, [b"ACGT", b"A"], [0, 1]),
                      site(107, 108, [b"T", b"*", b"TGG"], [0, 2])]),
    "leading_indel_ignored": (region([(b"GGACGTTCGTAC", 0, "2I10M"), (b"GTTCGTAC", 0, "2D8M")]),
                              [site(104, 105, [b"A", b"T"], [0, 1, 1])]),
    "leading_softclip": (region([(b"GGGTTCGTAC", 3, "3S7M")]), [site(104, 105, [b"A", b"T"], [0, 1])]),
    "eight_alleles": (region(EIGHT), [SKIPPED]),
    "seven_alleles": (region(EIGHT[:2] + EIGHT[3:]),
                      [site(104, 105, [b"A", b"AA", b"AC", b"AG", b"AT", b"C", b"G"], [0, 5, 6, 1, 2, 3, 4])]),
    "outside_origin": (region([(b"AGGTTCGAAC", 0, "10M")], origin=(103, 106)), [site(104, 105, [b"A", b"T"], [0, 1])]),
    # begin 0 and 1: the window [begin - 2, loc_end + 2) is cut at the contig's first base (the reference
    # throws there): [0, 3) and [0, 4) are overlapped by [0,50) and [2,9), [3,9) only by the latter; begin 2 as usual
    "begin_below_2": (region([(b"CGTTACGTAC", 0, "10M")], pb=0, reads=((0, 50), (2, 9), (3, 9), (4, 9))),
                      [site(0, 1, [b"A", b"C"], [0, 1], keep=[0, 1]), site(1, 2, [b"C", b"G"], [0, 1], keep=[0, 1, 2]),
                       site(2, 3, [b"G", b"T"], [0, 1], keep=[0, 1, 2, 3])]),
    "zero_reads": (region([(b"ACGTTCGTAC", 0, "10M")], reads=()), [site(104, 105, [b"A", b"T"], [0, 1], keep=[])]),
}


def shape_region(seed, window, n_haps, n_reads):
    """Reference path plus SNP haplotypes (one of them with a deletion when it fits)."""
    rng = np.random.default_rng(seed)
    ref = G.ACGT[rng.integers(0, 4, window)].tobytes()
    haps = []
    for h in range(1, n_haps):
        pos = sorted(set(rng.integers(0, window, max(1, window // 20)).tolist()))
        edits = [(p, 0, "S", int([b for b in G.ACGT if b != ref[p]][h % 3])) for p in pos]
        if h == 2 and window >= 20:
            edits = sorted(edits + [(window // 2, 2, "D", min(5, window // 4))])
        bases, cigar, _ = G.apply_edits(ref, edits)
        haps.append((bases, 0, cigar))
    if n_haps == 1:   # a lone haplotype that differs from the window
        haps, only = [], bytes([G.ACGT[(list(G.ACGT).index(ref[0]) + 1) % 4]]) + ref[1:]
        r = region([], ref=ref, pb=500, reads=[(480 + 3 * k, 520 + 3 * k) for k in range(n_reads)], seed=seed)
        r["haps"] = [dict(bases=only, begin=0, cigar=f"{window}M")]
        r["L"] = np.ascontiguousarray(r["L"][:, :1])
        return r
    return region(haps, ref=ref, pb=500, reads=[(480 + 3 * k, 520 + 3 * k) for k in range(n_reads)], seed=seed)


def alternating_runs():
    """1M1I1M1D x 50 then 10M: 201 one-base runs, a few of the M bases mismatching."""
    rng = np.random.default_rng(8)
    ref = G.ACGT[rng.integers(0, 4, 160)].tobytes()
    out, rp, cigar = bytearray(), 0, ""
    for k in range(50):
        for op in "MIMD":
            cigar += "1" + op
            if op == "M":
                out.append(ref[rp] if rng.random() < 0.8 else int(G.ACGT[(list(G.ACGT).index(ref[rp]) + 1) % 4]))
                rp += 1
            elif op == "I":
                out.append(int(G.ACGT[rng.integers(0, 4)]))
            else:
                rp += 1
    out += ref[rp:]
    return region([(bytes(out), 0, cigar + f"{len(ref) - rp}M")], ref=ref, pb=300, reads=((250, 400), (320, 340)))


def all_mismatches():
    rng = np.random.default_rng(9)
    ref = G.ACGT[rng.integers(0, 4, 300)].tobytes()
    alt = bytes(int(G.ACGT[(list(G.ACGT).index(b) + 1 + k % 3) % 4]) for k, b in enumerate(ref))
    return region([(alt, 0, "300M")], ref=ref, pb=7, reads=((0, 400), (100, 120), (290, 310)))


def lane_boundary():
    """One M run whose only mismatches sit at offsets 63 and 64."""
    rng = np.random.default_rng(10)
    ref = G.ACGT[rng.integers(0, 4, 130)].tobytes()
    alt = bytearray(ref)
    for p in (63, 64):
        alt[p] = int(G.ACGT[(list(G.ACGT).index(ref[p]) + 2) % 4])
    return region([(bytes(alt), 0, "130M")], ref=ref, pb=1000, reads=((1000, 1100),))


def shapes():
    out = {f"haps_{n}": shape_region(20 + n, 90, n, 30) for n in (1, 64, 65, 128)}
    out.update({f"reads_{n}": shape_region(40 + n, 90, 5, n) for n in (0, 1, 64, 65)})
    out["window_1"] = region([(b"C", 0, "1M")], ref=b"A", pb=50, reads=((40, 60), (52, 60), (53, 60)))
    out["window_1023"] = shape_region(60, 1023, 6, 20)
    out["alternating_runs"] = alternating_runs()
    out["all_mismatches"] = all_mismatches()
    out["lane_boundary"] = lane_boundary()
    return out


@pytest.fixture(scope="module")
def random_set():
    return G.regions(24, 415, 245, (8, 32), (50, 120), seed=71)


@pytest.fixture(scope="module")
def random_expected(random_set, gt_oracle_lib):
    return RS.call_regions(random_set, gt_oracle_lib)


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_hand_cases(gt_oracle_lib, name):
    reg, exp = HAND[name]
    got = RS.call_region(reg, gt_oracle_lib)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if e is SKIPPED:
            assert g["status"] == RS.TOO_MANY_ALLELES and g["n_alleles"] == 8 and g["begin"] == 104
            continue
        assert g["status"] != RS.TOO_MANY_ALLELES
        assert (g["begin"], g["loc_end"], g["alleles"], g["hap_allele"].tolist(), g["keep"].tolist()) == \
            (e["begin"], e["loc_end"], e["alleles"], e["hap_allele"], e["keep"])
        assert g["n_alleles"] == len(e["alleles"])


def test_random_set_covers_every_outcome(random_expected):
    recs = random_expected
    assert any(b"*" in r["alleles"] for r in recs), "no spanning deletion"
    assert any(r["n_alleles"] >= 3 and r["status"] != RS.TOO_MANY_ALLELES for r in recs), "no multi-allelic site"
    assert any(r["status"] == RS.HOM_REF for r in recs), "no hom-ref skip"
    assert any(r["status"] == RS.LOW_QUALITY_HET for r in recs), "no low-quality het"
    assert any(r["status"] == RS.EMITTED and r["a1"] == r["a2"] for r in recs), "no emitted hom-var"
    assert any(r["status"] == RS.EMITTED and r["a1"] != r["a2"] for r in recs), "no emitted het"


def test_generator_cigars_fit_their_haplotypes(random_set):
    import re
    starts = set()
    for reg in random_set:
        for h in reg["haps"]:
            ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDS])", h["cigar"])]
            assert "".join(f"{n}{op}" for n, op in ops) == h["cigar"]
            assert sum(n for n, op in ops if op in "MIS") == len(h["bases"])
            assert h["begin"] + sum(n for n, op in ops if op in "MD") <= len(reg["ref"])
            starts.add((h["begin"] > 0, ops[0][1] == "S", ops[-1][1] == "S"))
    assert {s[0] for s in starts} == {False, True} and any(s[1] for s in starts) and any(s[2] for s in starts)


def test_region_symbols_exported_and_no_fallback():
    import hcgt
    import hcphmm
    syms = hcgt.declared_symbols()
    assert {"hc_gt_call_regions", "hc_gt_calls_sites", "hc_gt_calls_free"} <= set(syms)
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert all(f" T {s}" in out for s in syms)
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(hcgt.GTError) as e:
        hcgt.call_regions([HAND["snp_het"][0]])
    assert e.value.code == hcphmm.ENODEV


# ---- GPU ----

@pytest.mark.gpu
def test_gpu_hand_cases(gt_oracle_lib):
    import hcgt
    regs = [HAND[k][0] for k in sorted(HAND)]
    RS.assert_same(hcgt.call_regions(regs), RS.call_regions(regs, gt_oracle_lib))


@pytest.mark.gpu
def test_gpu_random_set(random_set, random_expected):
    import hcgt
    RS.assert_same(hcgt.call_regions(random_set), random_expected)


@pytest.mark.gpu
def test_gpu_smallest_shapes(gt_oracle_lib):
    import hcgt
    for name, reg in shapes().items():
        exp = RS.call_region(reg, gt_oracle_lib)
        assert exp, name
        try:
            RS.assert_same(hcgt.call_regions([reg]), exp)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None


@pytest.mark.gpu
def test_gpu_same_arithmetic_as_genotype_sites(random_set):
    """The returned keep / hap_allele / n_alleles through the per-site entry
    point give the same bits: the two entry points share the arithmetic."""
    import hcgt
    recs = [r for r in hcgt.call_regions(random_set) if r["status"] != RS.TOO_MANY_ALLELES]
    sites = [dict(m=r["region"], keep=r["keep"], hap_allele=r["hap_allele"], n_alleles=r["n_alleles"]) for r in recs]
    again = hcgt.genotype_sites([reg["L"] for reg in random_set], sites)
    for r, (gl, gi, gq) in zip(recs, again):
        assert np.array_equal(gl.view(np.uint64), r["genotype_likelihoods"].view(np.uint64))
        assert (gi, gq) == (r["genotype_index"], r["genotype_quality"])


@pytest.mark.gpu
def test_gpu_deterministic(random_set):
    import hcgt
    RS.assert_same(hcgt.call_regions(random_set), hcgt.call_regions(random_set))


def _bad(name):
    reg = copy.deepcopy(HAND["deletion"][0])
    h = reg["haps"][1]   # ACGTAAC, 5M3D2M
    if name == "operator":
        h["cigar"] = "5M3N2M"
    elif name == "malformed":
        h["cigar"] = "5M3D2"
    elif name == "zero_run":
        h["cigar"] = "5M0I3D2M"
    elif name == "hap_length":
        h["cigar"] = "5M3D3M"
    elif name == "past_window":
        h["cigar"], h["bases"] = "5M6D2M", h["bases"]
    elif name == "begin_past_window":
        h["begin"] = 4
    elif name == "origin_before":
        reg["origin_begin"] = PB - 1
    elif name == "origin_after":
        reg["origin_end"] = PB + len(REF) + 1
    elif name == "origin_reversed":
        reg["origin_begin"], reg["origin_end"] = PB + 5, PB + 4
    elif name == "too_many_haps":
        reg["haps"] = reg["haps"][:1] * 129
        reg["L"] = np.zeros((1, 129))
    return reg


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["operator", "malformed", "zero_run", "hap_length", "past_window",
                                  "begin_past_window", "origin_before", "origin_after", "origin_reversed",
                                  "too_many_haps"])
def test_gpu_bad_input_rejected(gt_oracle_lib, name):
    import hcgt
    import hcphmm
    with pytest.raises(hcgt.GTError) as e:
        hcgt.call_regions([HAND["snp_het"][0], _bad(name)])
    assert e.value.code == hcphmm.EINVAL and "region 1" in str(e.value)
    good = [HAND["deletion_spans_snp"][0]]
    RS.assert_same(hcgt.call_regions(good), RS.call_regions(good, gt_oracle_lib))


@pytest.mark.gpu
def test_gpu_null_arguments():
    import ctypes as C

    import hcgt
    import hcphmm
    L = hcgt.lib()
    assert L.hc_gt_call_regions(None, 1, C.byref(C.c_void_p())) == hcphmm.EINVAL
    p = hcgt.PreparedRegions([HAND["snp_het"][0]])
    assert L.hc_gt_call_regions(p.arr, 1, None) == hcphmm.EINVAL
    p.arr[0].ref = None
    assert L.hc_gt_call_regions(p.arr, 1, C.byref(C.c_void_p())) == hcphmm.EINVAL
    assert L.hc_phmm_last_error()


@pytest.mark.gpu
def test_gpu_realistic_cigars(random_set, sw_oracle_lib, gt_oracle_lib):
    """The haplotypes of 4 regions re-aligned by the Smith-Waterman oracle."""
    import hcgt
    import sw_workloads as SWW
    regs = copy.deepcopy(random_set[:4])
    for reg in regs:
        off, cigars = sw_oracle_lib.batch(SWW.from_pairs([(reg["ref"], h["bases"]) for h in reg["haps"]]))
        for h, o, c in zip(reg["haps"], off, cigars):
            h["begin"], h["cigar"] = int(o), c
    RS.assert_same(hcgt.call_regions(regs), RS.call_regions(regs, gt_oracle_lib))
