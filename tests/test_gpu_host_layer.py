"""The host layer the seven stage engines share (csrc/stage_host.hpp: aligner,
genotyper, region caller, assembler, read preparation, SAM parser and contig
caller, with the window caller that chains them; and the region frame of
gt_engine_internal.hpp): buffers that grow, buffers that are released and made
again by a shutdown and the next call's init, and one frame with one set of
error texts behind hc_gt_call_regions and hc_region_call.

Every entry point goes through its Python wrapper. One fixture makes all the
calls once, in this order, and the tests compare what it kept:

    shutdown, init            every buffer empty
    tiny, large, tiny         the large call regrows every buffer
    shutdown, init, tiny      buffers released and made again
    shutdown, init, large     the large call into fresh buffers
"""
import numpy as np
import pytest

import asm_cases
import call_cases as CC
import gt_workloads as GW
import region_workloads as RW
import sam_cases as SC
import sw_workloads as SWW

pytestmark = pytest.mark.gpu

ENTRIES = ("hc_sw_align_flat", "hc_gt_genotype_sites", "hc_gt_call_regions", "hc_region_call", "hc_asm_assemble",
           "hc_prep_reads", "hc_sam_parse", "hc_call_windows", "hc_contig_call")


def _bits(x):
    """A result as nested lists of plain values, floats and arrays by their bytes."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, float):
        return np.float64(x).tobytes()
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    return x


def _windows(n, seed, n_reads):
    """n windows of call_cases.windows that have reads (its window 2 has none),
    window k cut to its first n_reads(k) reads."""
    wins = [w for w in CC.windows(n + 1 if n > 2 else n, seed=seed, reads_per_window=54) if w["reads"]][:n]
    return [dict(w, reads=w["reads"][:n_reads(k)]) for k, w in enumerate(wins)]


def _contig(n_windows, seed, n_reads):
    """(SAM text, reference) of a contig of n_windows windows of sam_cases.REGION
    bases: window k has n_reads(k) reads of 60 bases that cover its middle, every
    other one with a SNP there."""
    rng = np.random.default_rng(seed)
    ref = CC._bases(rng, n_windows * SC.REGION)
    hap = bytearray(ref)
    lines = []
    for w in range(n_windows):
        v = w * SC.REGION + 120
        hap[v] = CC.ACGT[(CC.ACGT.index(ref[v]) + 1) % 4]
        for j in range(n_reads(w)):
            at = v - 55 + j
            src = ref if j % 2 == 0 else bytes(hap)
            lines.append(SC.line(qname=f"w{w}r{j}", pos=at + 1, seq=src[at:at + 60].decode(), flag=(99, 147)[j % 2]))
    order = rng.permutation(len(lines))
    return (SC.HEADER + "".join(lines[k] + "\n" for k in order)).encode(), ref


def _inputs():
    """Per entry point (tiny, large, size): tiny is one region, two haplotypes and
    four reads (the aligner: two pairs); large is eight regions of a few dozen
    reads. size(input) is what the workspaces scale with; the test asserts that
    it more than doubles, so the large call cannot fit the quarter of slack."""
    reads = (24, 48)
    sw = (SWW.regions(1, 2, (60, 80), seed=901), SWW.regions(8, 8, (300, 415), seed=902), SWW.cells)
    gs = (GW.sites(1, 2, reads=(4, 4), haps=(2, 2), seed=903), GW.sites(8, 8, reads=reads, haps=(4, 8), seed=904),
          lambda x: sum(m.size for m in x[0]) + sum(len(s["keep"]) for s in x[1]))
    gr = (GW.regions(1, haps=(2, 2), reads=(4, 4), seed=905), GW.regions(8, haps=(8, 16), reads=reads, seed=906),
          lambda x: sum(r["L"].size + len(r["ref"]) * len(r["haps"]) for r in x))
    rc = (RW.regions(1, seed=907, n_variants=(1, 1), n_reads=(4, 4), artefact=False),
          RW.regions(8, seed=908, n_reads=reads),
          lambda x: sum((len(r["reads"]) + len(r["ref"])) * len(r["haps"]) for r in x))
    am = ([asm_cases.random_region(909, reads=(4, 4))], [asm_cases.random_region(910 + k, reads=reads) for k in range(8)],
          lambda x: sum(len(r["ref"]) + sum(len(b) for b, _ in r["reads"]) for r in x))
    # one window with four reads / eight windows of 24 to 45: as windows, and as the SAM text of a contig
    few, many = (lambda k: 4), (lambda k: 24 + 3 * k)
    cw = (_windows(1, 920, few), _windows(8, 921, many), lambda x: sum(len(w["reads"]) for w in x))
    pr = tuple([CC.prep_window(w) for w in x] for x in cw[:2]) + (cw[2],)
    ct = (_contig(1, 922, few), _contig(8, 923, many), lambda x: len(x[0]))
    sm = (ct[0][0], ct[1][0], len)
    return dict(zip(ENTRIES, (sw, gs, gr, rc, am, pr, sm, cw, ct)))


@pytest.fixture(scope="module")
def runs(engine):
    import hcasm
    import hccall
    import hccontig
    import hcgt
    import hcprep
    import hcregion
    import hcsw
    call = {
        "hc_sw_align_flat": hcsw.align_flat,
        "hc_gt_genotype_sites": lambda x: hcgt.genotype_sites(*x),
        "hc_gt_call_regions": hcgt.call_regions,
        "hc_region_call": lambda x: hcregion.call_regions(x, want_L=True, want_site_reads=True, want_cigars=True),
        "hc_asm_assemble": lambda x: hcasm.assemble(x, want_graph=True),
        "hc_prep_reads": hcprep.prep_reads,
        "hc_sam_parse": hccontig.parse_sam,
        "hc_call_windows": lambda x: hccall.call_windows(x, want_L=True, want_site_reads=True, want_cigars=True),
        "hc_contig_call": lambda x: hccontig.call_contig(x[0], SC.CONTIG, x[1], want_site_reads=True),
    }
    inputs = _inputs()

    def every(which):
        return {e: _bits(call[e](inputs[e][which])) for e in ENTRIES}

    def restart():
        engine.shutdown()
        engine.init(0)

    restart()
    out = dict(inputs=inputs)
    out["tiny"], out["large"], out["tiny_again"] = every(0), every(1), every(0)
    restart()
    out["tiny_reinit"] = every(0)
    restart()
    out["large_fresh"] = every(1)
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_large_input_outgrows_the_slack(runs, entry):
    tiny, large, size = runs["inputs"][entry]
    assert size(large) >= 2 * size(tiny) > 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_results_are_not_empty(runs, entry):
    """The comparisons below compare something: every call produced records."""
    for which in ("tiny", "large"):
        r = runs[which][entry]
        r = (r["sites"] if entry == "hc_region_call" else r[1] if entry == "hc_sw_align_flat"
             else r["records"][2] if entry == "hc_sam_parse" else r["windows"] if entry in ("hc_call_windows", "hc_contig_call")
             else r)
        assert len(r) > 0, which


@pytest.mark.parametrize("entry", ENTRIES)
def test_tiny_after_regrow_is_bit_identical(runs, entry):
    assert runs["tiny_again"][entry] == runs["tiny"][entry]


@pytest.mark.parametrize("entry", ENTRIES)
def test_regrown_large_equals_fresh_large(runs, entry):
    assert runs["large"][entry] == runs["large_fresh"][entry]


@pytest.mark.parametrize("entry", ENTRIES)
def test_tiny_after_release_and_reinit_is_bit_identical(runs, entry):
    assert runs["tiny_reinit"][entry] == runs["tiny"][entry]


# ---- one frame, one set of error texts ----

def _null_ref(reg, hap):
    reg.ref = None


def _ref_len_0(reg, hap):
    reg.ref_len = 0


def _n_haps_0(reg, hap):
    reg.n_haps = 0


def _origin_outside(reg, hap):
    reg.origin_end = reg.padded_begin + reg.ref_len + 1


def _hap_length_0(reg, hap):
    hap.length = 0


def _begin_beyond_ref(reg, hap):
    hap.alignment_begin = reg.ref_len + 1


def _bad_cigar(reg, hap):
    hap.cigar = b"12Q3M"


# (what is wrong with region 1 of two, the text both entry points give: recorded from the parent commit)
BAD_REGIONS = [
    (_null_ref, "region 1: null pointer"),
    (_ref_len_0, "region 1: ref_len, n_haps or n_reads out of range"),
    (_n_haps_0, "region 1: ref_len, n_haps or n_reads out of range"),
    (_origin_outside, "region 1: origin outside the padded window"),
    (_hap_length_0, "region 1 haplotype 0: length or alignment_begin out of range"),
    (_begin_beyond_ref, "region 1 haplotype 0: length or alignment_begin out of range"),
    (_bad_cigar, "region 1 haplotype 0: bad CIGAR '12Q3M'"),
]


@pytest.fixture(scope="module")
def two_regions():
    """Two good regions with aligned haplotypes, as both entry points take them
    (the region caller's copy has no reads: the frame is checked before any)."""
    gt = GW.regions(2, haps=(2, 2), reads=(4, 4), seed=911)
    none = np.zeros(0, np.int64)
    return gt, [dict(r, reads=[], read_begin=none, read_end=none) for r in gt]


@pytest.mark.parametrize("spoil,text", BAD_REGIONS, ids=[s.__name__[1:] for s, _ in BAD_REGIONS])
def test_bad_region_same_error_from_both_entry_points(engine, two_regions, spoil, text):
    import hcgt
    import hcregion
    gt, rc = two_regions
    p = hcgt.PreparedRegions(gt)
    spoil(p.arr[1], p.arr[1].haps[0])
    with pytest.raises(hcgt.GTError) as e:
        p.free(p.run())
    assert e.value.code == engine.EINVAL
    assert str(e.value) == f"hc_gt error {engine.EINVAL}: {text}"
    q = hcregion.Prepared(rc)
    spoil(q.arr[1], q.arr[1].haps[0])
    with pytest.raises(hcregion.RegionError) as e:
        q.free(q.run(hcregion.flags_of()))
    assert e.value.code == engine.EINVAL
    assert str(e.value) == f"hc_region error {engine.EINVAL}: {text}"
