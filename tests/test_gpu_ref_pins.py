"""GPU: the device side of every stage against the REFERENCE's recorded results
(tests/golden/chain_golden.npz, made by the reference's own headers compiled in
place; see test_ref_pins.py). Nothing here goes through a restatement: the SAM
parse, the read preparation, the aligner, compute_likelihoods, the genotyper,
the one-call region chain and the contig caller's VCF lines are compared with
the fixture directly, doubles as bits. The inputs on which the library
deliberately does not do what the reference does are the rows of
test_ref_pins.DEVIATIONS, under the same rules."""
import numpy as np
import pytest

import pin_cases as P
import sw_workloads as SWW
import test_ref_pins as T

pytestmark = pytest.mark.gpu

EMITTED, TOO_MANY_ALLELES = 0, 3


@pytest.fixture(scope="module")
def fixture():
    return P.load_fixture()


def _enc(s):
    return s.encode("latin-1")


# ---- parse -----------------------------------------------------------------------------

def test_parse_sam_reads_what_the_reference_reads(engine, fixture, monkeypatch):
    import hccontig
    text, expected, exp = T.parse_text(fixture, "library")
    assert len(expected) > 900 and sum(e == "skip" for _, e in exp) >= 20
    met = {r["name"] for c in fixture["parse"] for r in T.rows_for("parse", "library", c["input"], c["output"])}
    assert met == T.table_rows("parse", "library")
    whole = hccontig.parse_sam(text)
    T.check_parsed_text(text, whole, expected, "one text")
    monkeypatch.setenv("HC_SAM_STAGE_BYTES", "4096")
    assert len(text) > 20 * 4096
    T.check_parsed_text(text, hccontig.parse_sam(text), expected, "4096-byte pieces")


def test_parse_sam_refuses_where_the_reference_fails_or_the_table_says_so(engine, fixture):
    import hccontig
    import hcphmm
    bad = [c for c in fixture["parse"] if T.parse_expectation(c, "library") == "error"]
    assert len(bad) >= 40 and any(not c["output"]["fail"] for c in bad) and any(c["output"]["fail"] for c in bad)
    for c in bad:
        with pytest.raises(hccontig.ContigError) as e:
            hccontig.parse_sam(_enc("a 0 b 1 0 1M = 0 0 A I\n" + c["input"] + "\n"))
        assert e.value.code == hcphmm.EINVAL and e.value.msg.startswith("line 2: "), (c["name"], e.value.msg)


# ---- prepare ---------------------------------------------------------------------------

def _ref_len(cigar):
    return sum(int(n) for n, op in T.CIGAR_RE.findall(cigar) if op in "MDN=X")


def _prep_expected(x, out):
    """hc_prep_record fields from the reference's strings. A read the minimum-length
    filter erased left no state behind: only keep and drop_reason are known."""
    recs = []
    for r, o in zip(x["reads"], out["reads"]):
        if o["left"]:
            e = dict(keep=0, drop_reason=o["reason"])
            if o["reason"] != 5:
                e.update(offset=0, length=len(r["seq"]), new_pos=r["pos"], front_to_M=0, back_to_M=0, begin=0, end=0)
            recs.append(e)
            continue
        old, new = T.CIGAR_RE.findall(r["cigar"]), T.CIGAR_RE.findall(o["CIGAR"])
        front, back = int(new[0] != old[0]), int(new[-1] != old[-1])
        if len(old) == 1 and front:   # one element is front() and back(): the reverse strand rewrites it as back()
            front, back = (0, 1) if r["flag"] & 0x10 else (1, 0)
        assert o["QUAL"] == P.qual_of(len(r["seq"]))[ord(o["SEQ"][0]) - 33:][:len(o["SEQ"])]
        recs.append(dict(keep=1, drop_reason=0, offset=ord(o["SEQ"][0]) - 33, length=len(o["SEQ"]), new_pos=o["POS"],
                         front_to_M=front, back_to_M=back, begin=o["POS"] - 1, end=o["POS"] - 1 + _ref_len(o["CIGAR"])))
    return recs


def test_prep_reads_does_what_the_reference_does(engine, fixture):
    import hcprep
    cases = [c for c in fixture["prepare"] if not T.rows_for("prepare", "library", c["input"], c["output"])]
    assert len(cases) >= 40 and not any(c["output"]["threw"] for c in cases)
    got = hcprep.prep_reads([P.prep_window(c["input"]) for c in cases])
    for c, g in zip(cases, got):
        exp = _prep_expected(c["input"], c["output"])
        assert len(g["records"]) == len(exp), c["name"]
        for k, (a, e) in enumerate(zip(g["records"], exp)):
            assert {f: a[f] for f in e} == e, (c["name"], k, a, e)
        kept = [k for k, e in enumerate(exp) if e["keep"]]
        assert (g["kept"], g["n_kept"], g["kept_bases"]) == (kept, len(kept), sum(exp[k]["length"] for k in kept)), c["name"]


def test_prep_reads_refuses_what_the_table_says(engine, fixture):
    import hcphmm
    import hcprep
    met = set()
    for c in fixture["prepare"]:
        rows = T.rows_for("prepare", "library", c["input"], c["output"])
        if not rows:
            continue
        for r in rows:
            met.add(r["name"])
            assert T.admissible(r, c["output"]) is None, (c["name"], r["name"])
        with pytest.raises(hcprep.PrepError) as e:
            hcprep.prep_reads([P.prep_window(c["input"])])
        assert e.value.code == hcphmm.EINVAL and "window 0 read 1:" in e.value.msg, c["name"]
    assert met == T.table_rows("prepare", "library")


# ---- align -----------------------------------------------------------------------------

def test_aligner_equals_the_reference(engine, fixture):
    import hcsw
    cases = fixture["align"]
    assert not any(c["output"]["threw"] for c in cases)
    for params in sorted({tuple(c["input"]["params"]) for c in cases}):
        mine = [c for c in cases if tuple(c["input"]["params"]) == params]
        off, cig = hcsw.align_flat(SWW.from_pairs([(_enc(c["input"]["ref"]), _enc(c["input"]["alt"])) for c in mine]),
                                   params=params)
        for c, o, g in zip(mine, off, cig):
            assert (int(o), g) == (c["output"]["offset"], c["output"]["cigar"]), c["name"]


# ---- likelihoods -----------------------------------------------------------------------

def _reads(x):
    return [(_enc(s), _enc(q), b"I" * len(s), b"I" * len(s), b"+" * len(s)) for s, q in x["reads"]]


def test_compute_likelihoods_equals_the_reference(engine, fixture):
    import hcphmm
    for c in fixture["likelihoods"]:
        x, out = c["input"], c["output"]
        reads, haps = _reads(x), [_enc(h) for h in x["haps"]]
        raw = hcphmm.cross(reads, haps, use_double=False)
        assert P.same_bits(raw, out["raw"]), (c["name"], "before normalisation")
        L, kept = hcphmm.compute_likelihoods(haps, reads, use_double=False)
        ids = {id(r) for r in kept}
        assert [k for k, r in enumerate(reads) if id(r) in ids] == [int(k) for k in out["kept"]], c["name"]
        assert P.same_bits(L, out["L"]), c["name"]


def test_region_finish_equals_the_reference(engine, fixture):
    import hcregion
    cases = fixture["normalize"]
    got = hcregion.finish([c["input"]["L"] for c in cases], [c["input"]["read_len"] for c in cases])
    for c, (L, keep, _order) in zip(cases, got):
        assert np.flatnonzero(keep).tolist() == [int(k) for k in c["output"]["kept"]], c["name"]
        assert P.same_bits(L, c["output"]["L"]), c["name"]


# ---- genotype --------------------------------------------------------------------------

def _check_sites(name, region, recs, out):
    """Every record field against the reference's site; a site on which the reference
    throws (the table's row) against the rule of include/hc_gt.h."""
    assert [m["begin"] for m in recs] == [s["begin"] for s in out["sites"]], name
    for m, s in zip(recs, out["sites"]):
        if s["threw"]:
            assert s["begin"] < 2, name
            rb, re_ = region["read_begin"], region["read_end"]
            keep = [k for k in range(len(rb)) if rb[k] < m["loc_end"] + 2 and 0 < re_[k]]
            assert list(m["keep"]) == keep and m["status"] != TOO_MANY_ALLELES, (name, s["begin"])
            continue
        why = T._site_differs(m, s)
        assert why is None, (name, s["begin"], why)


def test_call_regions_equals_the_reference_on_every_field(engine, fixture):
    import hcgt
    cases = fixture["genotype"]
    regions = [c["input"] for c in cases]
    assert sum(len(c["output"]["sites"]) for c in cases) >= 60
    recs = hcgt.call_regions(regions)
    met = set()
    for k, c in enumerate(cases):
        mine = [m for m in recs if m["region"] == k]
        _check_sites(c["name"], c["input"], mine, c["output"])
        rows = T.rows_for("genotype", "library", c["input"], c["output"])
        met |= {r["name"] for r in rows}
        if rows:
            assert c["output"]["whole_call_threw"] and all(T.admissible(r, c["output"]) is None for r in rows), c["name"]
            continue
        assert not c["output"]["whole_call_threw"], c["name"]
        assert T._emitted(mine) == T._variants(c["output"]["variants"]), c["name"]
    assert met == T.table_rows("genotype", "library")


# ---- chain -----------------------------------------------------------------------------

def _prepared(x, out):
    """The reads the reference's filter_reads / hard_clip_reads left, as chain_region takes them."""
    return [(o["SEQ"], o["QUAL"], o["POS"] - 1, o["POS"] - 1 + _ref_len(o["CIGAR"])) for o in out["prepared"] if not o["left"]]


def test_region_call_equals_the_reference_chain(engine, fixture):
    import hcregion
    cases = [c for c in fixture["chain"] if c["output"]["threw"] or c["output"]["outcome"] == 0]
    regs = [T.chain_region(c["input"], _prepared(c["input"], c["output"])) for c in cases]
    got = hcregion.call_regions(regs, want_L=True, want_site_reads=True, want_cigars=True)
    called = 0
    for k, c in enumerate(cases):
        sites = [s for s in got["sites"] if s["region"] == k]
        if T.rows_for("chain", "library", c["input"], c["output"]):
            assert c["output"]["threw"] and any(s["begin"] < 2 for s in sites), c["name"]
            continue
        assert int(got["keep"][k].sum()) == c["output"]["n_reads"], c["name"]
        assert T._emitted(sites) == T._variants(c["output"]["variants"]), c["name"]
        called += len(c["output"]["variants"])
    assert called >= 8


def test_contig_caller_prints_what_variant_print_prints(engine, fixture):
    """The contig caller assembles its own haplotypes, so a line is compared where the
    caller emits a variant the reference chain emitted too: the same position, alleles,
    genotype and quality must be the same bytes as Variant::print's."""
    import hccontig
    import oracle
    case = next(c for c in fixture["chain"] if c["name"] == "whole_contig")
    x, out = case["input"], case["output"]
    sam = _enc("@HD\tVN:1.6\n" + "\n".join(oracle.sam_line(f"r{k}", r["flag"], r["pos"], r["mapq"], r["cigar"],
                                                            r["mate_same"], r["seq"], r["qual"])
                                            for k, r in enumerate(x["reads"])) + "\n")
    got = hccontig.call_contig(sam, oracle.CHAIN_CONTIG, _enc(x["ref"]), pick="first")
    lines = got["vcf"].decode("latin-1").splitlines(keepends=True)
    body = [ln for ln in lines if not ln.startswith("#")]
    emitted = [s for s in got["sites"] if s["status"] == EMITTED]
    assert len(body) == len(emitted)
    ref_lines = {(v["begin"], tuple(v["alleles"]), v["a1"], v["a2"], v["gq"]): v["text"] for v in out["variants"]}
    same = 0
    for s, ln in zip(emitted, body):
        key = (s["begin"], tuple(s["alleles"]), s["a1"], s["a2"], s["genotype_quality"])
        if key in ref_lines:
            assert ln == ref_lines[key], (ln, ref_lines[key])
            same += 1
    assert same >= 1, (body, sorted(ref_lines.values()))
