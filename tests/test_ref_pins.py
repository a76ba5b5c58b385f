"""CPU: every restated stage of the region chain against the REFERENCE compiled
in place (oracle/ref_chain_driver.cpp): the SAM parse, filter_reads /
hard_clip_reads, the aligner's front, compute_likelihoods' rescue loop,
normalisation and read filter, the whole of assign_genotype_likelihoods, the VCF
line and the chain of call_region behind the assembler.

The committed fixture (tests/golden/chain_golden.npz, written by
tests/golden/make_chain_golden.py) holds the inputs and what the reference did
with them; each restatement must give the same, field for field, doubles as
bits. Where oracle/_ref/libref_chain.so exists the same comparisons run live on
seeded random inputs.

DEVIATIONS is the one list of inputs on which the library (and with it the
restatement that is its expected side) does not do what the reference does. A
row is admissible only where the reference throws, leaves its stream in failbit
or defines no result, or where a public header of the library documents the
refusal; everything outside the table is exact. The tests fail when a case
deviates outside the table, when a row's case no longer deviates, when a row
sits on a case the reference finishes normally without a header saying so, and
when a row matches no case of the fixture at all."""
import os
import re

import numpy as np
import pytest

import gt_restate as RS
import pin_cases as P
import prep_restate as PR
import region_workloads as RW
import sam_restate as SR
import sw_workloads as SWW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACE = " \t\n\v\f\r"
CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")


# ---- the table -------------------------------------------------------------------------

def _tokens(line):
    return [t for t in re.split("[" + SPACE + "]+", line) if t][:11]


def _digits(t, signed=False):
    return bool(re.fullmatch(r"-?\d+" if signed else r"\d+", t))


def _integers_decimal(tok):
    return all(_digits(tok[k]) for k in (1, 3, 4, 7)) and _digits(tok[8], signed=True)


def _cigar_ok(t):
    runs = CIGAR_RE.findall(t)
    return "".join(a + b for a, b in runs) == t and bool(runs) and all(int(a) <= SR.MAX_CIGAR_LENGTH for a, _ in runs)


def _header(name, phrase):
    return ("header", name, phrase)


def _read_length(cigar):
    return sum(int(n) for n, op in CIGAR_RE.findall(cigar) if op in "MIS=X")


def row(stage, name, when, reference, library, basis, sides=("restatement", "library")):
    """sides: who deviates. The restatement follows the library except in the read
    preparation, where it follows the reference and the library refuses."""
    return dict(stage=stage, name=name, when=when, reference=reference, library=library, basis=basis, sides=sides)


def _unfiltered(x, pred):
    return any(r["mapq"] >= 20 and not r["flag"] & 0x500 and r["mate_same"] and pred(r) for r in x["reads"])


DEVIATIONS = [
    row("parse", "blank line",
        lambda x, o: not _tokens(x),
        "operator>> fails on QNAME; load_all_reads goes on with the record as it is",
        "the line is skipped: it has no record",
        _header("hc_sam.h", "A line without any field")),
    row("parse", "CIGAR *",
        lambda x, o: len(_tokens(x)) == 11 and _tokens(x)[5] == "*" and not o["fail"] and _integers_decimal(_tokens(x)),
        "to_cigar_elements makes one element of length '*' - '0' (as uint32) and operator NUL",
        "n_cigar = 0 and HC_SAM_DEFECT_NO_CIGAR",
        _header("hc_sam.h", '"*" alone is n_cigar = 0')),
    row("parse", "an integer field that is not decimal digits",
        lambda x, o: len(_tokens(x)) == 11 and not o["fail"] and not _integers_decimal(_tokens(x)),
        "num_get takes a leading '+' and stops at the first other character; the next field starts there",
        "HC_PHMM_EINVAL naming the field",
        _header("hc_sam.h", "decimal digits only")),
    row("parse", "a CIGAR that is not runs of digits and MIDNSHP=X, or a run above 2^28 - 1",
        lambda x, o: (len(_tokens(x)) == 11 and not o["fail"] and _integers_decimal(_tokens(x)) and _tokens(x)[5] != "*"
                      and not _cigar_ok(_tokens(x)[5])),
        "to_cigar_elements takes any character as an operator and wraps the length in uint32",
        "HC_PHMM_EINVAL naming CIGAR",
        _header("hc_sam.h", "one or more elements of digits")),
    row("prepare", "POS 0 behind no flag filter",
        lambda x, o: _unfiltered(x, lambda r: r["pos"] == 0),
        "get_alignment_begin() wraps to 2^32 - 1 and the read is clipped as one lying there",
        "HC_PHMM_EINVAL naming the window and the read",
        _header("hc_prep.h", "pos == 0"), sides=("library",)),
    row("prepare", "a CIGAR whose read length is not the length of SEQ, behind no flag filter",
        lambda x, o: _unfiltered(x, lambda r: _read_length(r["cigar"]) != len(r["seq"])),
        "substr clips bases that no S covers, or throws std::out_of_range",
        "HC_PHMM_EINVAL naming the window and the read",
        _header("hc_prep.h", "differs from seq_len"), sides=("library",)),
    row("genotype", "a site at contig position 0 or 1",
        lambda x, o: any(s["begin"] < 2 for s in o["sites"]),
        "expand_within_contig(2) wraps begin - 2 and Interval's constructor throws: the whole call ends",
        "the window is cut at the contig's first base: reads overlapping [0, loc_end + 2) are kept",
        "throws"),
    row("chain", "a site at contig position 0 or 1",
        lambda x, o: o["threw"],
        "assign_genotype_likelihoods throws (the row above)",
        "the region is called",
        "throws"),
]


def rows_for(stage, side, x, out):
    return [r for r in DEVIATIONS if r["stage"] == stage and side in r["sides"] and r["when"](x, out)]


def admissible(row, out):
    """None when the row may stand on this case, else why not."""
    basis = row["basis"]
    if basis == "throws":
        threw = out["threw"] or out.get("whole_call_threw", False)
        return None if threw else "the reference finishes normally on this input"
    name, phrase = basis[1], basis[2]
    text = " ".join(open(os.path.join(ROOT, "include", name)).read().replace("*", " ").split())
    want = " ".join(phrase.replace("*", " ").split())
    return None if want in text else f"include/{name} does not say {phrase!r}"


# ---- one comparison per stage: None when restatement and reference agree ---------------

def _cmp(label, mine, ref):
    return None if mine == ref else f"{label}: {mine!r} != reference {ref!r}"


def cmp_parse(x, out, libs):
    try:
        r = SR.parse_record(x)
    except SR.SamSyntax as e:
        return None if out["fail"] else f"SamSyntax({e.field}) where the reference parses"
    if r is None:
        return "no record where the reference " + ("fails" if out["fail"] else "parses")
    if out["fail"]:
        return "a record where the reference fails"
    seq, qual = x[r["seq_off"]:r["seq_off"] + r["seq_len"]], x[r["qual_off"]:r["qual_off"] + r["qual_len"]]
    mine = (r["flag"], r["pos"], r["mapq"], [(n, op) for n, op in r["elements"]], r["mate_same_contig"], seq, qual)
    ref = (out["FLAG"], out["POS"], out["MAPQ"], [(n, op) for n, op in out["elements"]], int(out["RNEXT"] == "="),
           out["SEQ"], out["QUAL"])
    return _cmp("record", mine, ref)


def cmp_prepare(x, out, libs):
    sam = [PR.SAMRecord(r["flag"], r["pos"], r["mapq"], r["cigar"], "=" if r["mate_same"] else "chrOther", r["seq"],
                        r["qual"]) for r in x["reads"]]
    try:
        _, reasons = PR.prepare(sam, x["begin"], x["end"])
    except IndexError:
        return None if out["threw"] else "substr throws where the reference finishes"
    if out["threw"]:
        return "finishes where the reference throws"
    mine = [(c, c != PR.KEPT) + (() if c != PR.KEPT else (s.POS, PR.cigar_text(s.CIGAR), s.SEQ, s.QUAL))
            for s, c in zip(sam, reasons)]
    ref = [(r["reason"], r["left"]) + (() if r["left"] else (r["POS"], r["CIGAR"], r["SEQ"], r["QUAL"])) for r in out["reads"]]
    for k, (a, b) in enumerate(zip(mine, ref)):
        if a != b:
            return f"read {k}: {a!r} != reference {b!r}"
    return _cmp("reads", len(mine), len(ref))


def cmp_align(x, out, libs):
    off, cig = libs["sw"].batch(SWW.from_pairs([(x["ref"].encode("latin-1"), x["alt"].encode("latin-1"))]),
                                params=tuple(x["params"]), overhang=9, shortcut=True)
    if out["threw"]:
        return "finishes where the reference throws"
    return _cmp("alignment", (int(off[0]), cig[0]), (out["offset"], out["cigar"]))


def _pair_region(x):
    enc = lambda s: s.encode("latin-1")   # noqa: E731
    return dict(haps=[enc(h) for h in x["haps"]],
                reads=[(enc(s), enc(q), b"I" * len(s), b"I" * len(s), b"+" * len(s)) for s, q in x["reads"]])


def cmp_likelihoods(x, out, libs):
    r = _pair_region(x)
    nr, nh = len(r["reads"]), len(r["haps"])
    raw = libs["phmm"].pairs(RW.pair_batch(r), nthreads=1)["loglik"].reshape(nr, nh)
    if out["threw"]:
        return "finishes where the reference throws"
    if not P.same_bits(raw, out["raw"]):
        bad = np.argwhere(P.bits(raw) != P.bits(out["raw"]))[0]
        return f"pair {tuple(bad)} before normalisation: {raw[tuple(bad)]!r} != reference {out['raw'][tuple(bad)]!r}"
    L, keep = libs["phmm"].normalize(raw, np.array([len(s) for s, _ in x["reads"]], np.int32))
    if not np.array_equal(np.flatnonzero(keep), out["kept"]):
        return f"kept reads {np.flatnonzero(keep).tolist()} != reference {out['kept'].tolist()}"
    return None if P.same_bits(L[keep], out["L"]) else "normalised matrix differs"


def cmp_normalize(x, out, libs):
    L, keep = libs["phmm"].normalize(x["L"], np.array(x["read_len"], np.int32))
    if not np.array_equal(np.flatnonzero(keep), out["kept"]):
        return f"kept reads {np.flatnonzero(keep).tolist()} != reference {[int(k) for k in out['kept']]}"
    return None if P.same_bits(L[keep], np.asarray(out["L"]).reshape(-1, np.asarray(x["L"]).shape[1])) else "matrix differs"


def _site_differs(m, s):
    """A restated site record against the reference's site; None when equal."""
    if (m["begin"], m["loc_end"]) != (s["begin"], s["loc_end"]) or s["loc_begin"] != s["begin"]:
        return f"location [{m['begin']}, {m['loc_end']}) != reference [{s['loc_begin']}, {s['loc_end']})"
    if len(s["alleles"]) > RS.MAX_ALLELES:
        return _cmp("status", (m["status"], m["n_alleles"]), (RS.TOO_MANY_ALLELES, RS.MAX_ALLELES + 1))
    if m["status"] == RS.TOO_MANY_ALLELES:
        return "too many alleles where the reference has " + str(len(s["alleles"]))
    for key in ("alleles", "genotype_index", "genotype_quality"):
        if list(m[key]) != list(s[key]) if key == "alleles" else m[key] != s[key]:
            return f"{key}: {m[key]!r} != reference {s[key]!r}"
    for key in ("hap_allele", "keep"):
        if not np.array_equal(m[key], s[key]):
            return f"{key}: {list(m[key])} != reference {list(s[key])}"
    return None if P.same_bits(m["genotype_likelihoods"], s["genotype_likelihoods"]) else \
        f"genotype likelihoods: {m['genotype_likelihoods']} != reference {s['genotype_likelihoods']}"


def _emitted(recs):
    return [(m["begin"], m["loc_end"], list(m["alleles"]), m["a1"], m["a2"], m["genotype_quality"]) for m in recs
            if m["status"] == RS.EMITTED]


def _variants(vs):
    return [(v["begin"], v["end"], list(v["alleles"]), v["a1"], v["a2"], v["gq"]) for v in vs]


def _lines(recs):
    return [SR.variant_line("c", m["begin"], [a.decode("latin-1") for a in m["alleles"]], (m["a1"], m["a2"]),
                            m["genotype_quality"]) for m in recs if m["status"] == RS.EMITTED]


def cmp_genotype(x, out, libs):
    mine = RS.call_region(x, libs["gt"])
    if [m["begin"] for m in mine] != [s["begin"] for s in out["sites"]]:
        return f"sites {[m['begin'] for m in mine]} != reference {[s['begin'] for s in out['sites']]}"
    why = None
    for m, s in zip(mine, out["sites"]):
        if s["threw"]:
            why = why or f"site {s['begin']}: a record where the reference throws"
            continue
        d = _site_differs(m, s)
        if d:
            return f"site {s['begin']}: {d}"   # a real difference, whatever the table says
    if out["whole_call_threw"]:
        return why or "finishes where the reference throws"
    if why:
        return why
    if _emitted(mine) != _variants(out["variants"]):
        return f"emitted {_emitted(mine)} != reference {_variants(out['variants'])}"
    return _cmp("VCF lines", _lines(mine), [v["text"] for v in out["variants"]])


def chain_region(x, prepared):
    """The region hcregion.call_regions / region_chain.cpu_chain take, from prepared reads
    [(seq, qual, begin, end)]."""
    enc = lambda s: s.encode("latin-1")   # noqa: E731
    return dict(ref=enc(x["ref"]), padded_begin=x["padded_begin"], origin_begin=x["origin_begin"],
                origin_end=x["origin_end"], haps=[enc(h) for h in x["haps"]],
                reads=[(enc(s), enc(q), b"I" * len(s), b"I" * len(s), b"+" * len(s)) for s, q, _, _ in prepared],
                read_begin=np.array([p[2] for p in prepared], np.int64), read_end=np.array([p[3] for p in prepared], np.int64))


def cmp_chain(x, out, libs):
    import region_chain
    sam = [PR.SAMRecord(r["flag"], r["pos"], r["mapq"], r["cigar"], "=" if r["mate_same"] else "chrOther", r["seq"],
                        r["qual"]) for r in x["reads"]]
    kept, _ = PR.prepare(sam, x["padded_begin"], x["padded_begin"] + len(x["ref"]))
    if not kept or len(x["haps"]) <= 1:   # haplotypecaller.hpp:96,101
        mine = dict(outcome=1 if not kept else 2, n_reads=0, sites=[])
    else:
        reg = chain_region(x, [(s.SEQ, s.QUAL) + s.get_interval() for s in kept])
        got = region_chain.cpu_chain([reg], libs["phmm"], libs["sw"], libs["gt"])
        mine = dict(outcome=0, n_reads=int(got["keep"][0].sum()), sites=got["sites"])
    if out["threw"]:
        return "finishes where the reference throws"
    if (mine["outcome"], mine["n_reads"]) != (out["outcome"], out["n_reads"]):
        return f"outcome, reads {(mine['outcome'], mine['n_reads'])} != reference {(out['outcome'], out['n_reads'])}"
    if _emitted(mine["sites"]) != _variants(out["variants"]):
        return f"emitted {_emitted(mine['sites'])} != reference {_variants(out['variants'])}"
    return _cmp("VCF lines", _lines(mine["sites"]), [v["text"] for v in out["variants"]])


COMPARE = dict(parse=cmp_parse, prepare=cmp_prepare, align=cmp_align, likelihoods=cmp_likelihoods,
               normalize=cmp_normalize, genotype=cmp_genotype, chain=cmp_chain)


def check_cases(stage, side, rows, compare):
    """Every case exact or in the table; compare(input, reference output) gives None
    for agreement. Returns the names of the table rows that were met."""
    met, wrong = set(), []
    for case in rows:
        x, out = case["input"], case["output"]
        why = compare(x, out)
        table = rows_for(stage, side, x, out)
        if why and not table:
            wrong.append(f"{case['name']}: deviates outside the table: {why}")
        if table and not why:
            wrong.append(f"{case['name']}: row {table[0]['name']!r} no longer deviates")
        for r in table:
            met.add(r["name"])
            bad = admissible(r, out)
            if bad:
                wrong.append(f"{case['name']}: row {r['name']!r} may not stand: {bad}")
    assert not wrong, f"{len(wrong)} of {len(rows)} {stage} cases:\n" + "\n".join(wrong[:20])
    return met


def table_rows(stage, side):
    return {r["name"] for r in DEVIATIONS if r["stage"] == stage and side in r["sides"]}


def check_stage(stage, rows, libs):
    return check_cases(stage, "restatement", rows, lambda x, out: COMPARE[stage](x, out, libs))


# ---- fixtures --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture():
    return P.load_fixture()


@pytest.fixture(scope="module")
def libs(oracle_lib, sw_oracle_lib, gt_oracle_lib):
    return dict(phmm=oracle_lib, sw=sw_oracle_lib, gt=gt_oracle_lib)


@pytest.fixture(scope="module")
def reference():
    import oracle
    if not oracle.chain_reference_available():
        pytest.skip("oracle/_ref/libref_chain.so is not built (the reference tree is absent): "
                    "the committed fixture is the pin")
    return oracle.ChainReference()


# ---- the fixture form ------------------------------------------------------------------

@pytest.mark.parametrize("stage", P.STAGES)
def test_restatement_equals_the_reference_on_the_fixture(fixture, libs, stage):
    met = check_stage(stage, fixture[stage], libs)
    rows = table_rows(stage, "restatement")
    assert met == rows, f"table rows that no {stage} case of the fixture meets: {sorted(rows - met)}"


def test_fixture_holds_the_edges_it_is_there_for(fixture):
    """Read off the reference's outputs, so a regenerated fixture cannot lose them quietly."""
    out = {s: {c["name"]: c["output"] for c in fixture[s]} for s in P.STAGES}
    for s in P.STAGES:
        assert any(not o["threw"] for o in out[s].values()), s
    assert out["parse"]["err_pos_plus"]["fail"] == 0 and out["parse"]["err_pos_plus"]["POS"] == 1
    assert (out["align"]["equal_2_mismatches"]["offset"], out["align"]["equal_2_mismatches"]["cigar"]) == (0, "80M")
    sites = [s for o in out["genotype"].values() for s in o["sites"]]
    assert sorted({s["begin"] for s in sites if s["threw"]}) == [0, 1]
    assert all(s["threw"] for s in sites if s["begin"] < 2) and not any(s["threw"] for s in sites if s["begin"] >= 2)
    ok = [s for s in sites if not s["threw"] and "keep" in s]
    assert {2, 3, 7} <= {len(s["alleles"]) for s in ok} and any(len(s["alleles"]) > 7 for s in sites if not s["threw"])
    halves = [k for k in out["genotype"] if k.startswith("quality_on_")]
    assert len(halves) >= 3
    for k in halves:   # -10 * (second - best) sits on .5 in the reference's own likelihoods
        gl = sorted(out["genotype"][k]["sites"][0]["genotype_likelihoods"])
        assert -10 * (gl[-2] - gl[-1]) == float(k[len("quality_on_"):]), k
    # exact ties: the first comparison is >, the later ones >= (genotyper.hpp:334,348): the last of equals wins
    tie = out["genotype"]["tie_three_alleles_no_reads"]["sites"][0]
    assert len(set(P.bits(tie["genotype_likelihoods"]).tolist())) == 1 and tie["genotype_index"] == 5
    tie = out["genotype"]["tie_equal_columns"]["sites"][0]["genotype_likelihoods"]
    assert P.bits(tie)[0] == P.bits(tie)[2]
    norm = out["normalize"]
    assert len(norm["on_threshold"]["kept"]) == 9 and len(norm["below_threshold"]["kept"]) == 0
    lik = out["likelihoods"]
    assert len(lik["rescued_and_all_filtered"]["kept"]) == 0
    assert {o["outcome"] for o in out["chain"].values() if not o["threw"]} == {0, 1, 2}


def test_rescued_pairs_are_in_the_likelihood_fixture(fixture, libs):
    """The fp32 pass underflows on some pairs of the fixture, so the fp64 branch of the rescue loop is pinned."""
    case = next(c for c in fixture["likelihoods"] if c["name"] == "rescued_among_good")
    res = libs["phmm"].pairs(RW.pair_batch(_pair_region(case["input"])), nthreads=1)
    assert 0 < int(res["rescued"].sum()) < len(res["rescued"])


def parse_expectation(case, side):
    """"error", "skip" or the record the reference read, with the table's rows applied."""
    x, out = case["input"], case["output"]
    names = {r["name"] for r in rows_for("parse", side, x, out)}
    if "blank line" in names:
        return "skip"
    if names - {"CIGAR *"} or out["fail"]:
        return "error"
    words = [] if "CIGAR *" in names else [n << 4 | SR.OPS.index(op) for n, op in out["elements"]]
    enc = lambda t: t.encode("latin-1")   # noqa: E731
    return dict(flag=out["FLAG"], pos=out["POS"], mapq=out["MAPQ"], mate_same_contig=int(out["RNEXT"] == "="),
                seq=enc(out["SEQ"]), qual=enc(out["QUAL"]), words=words)


def check_parsed_text(text, parsed, expected, tag):
    """The records of a whole text (load_all_reads' or hc_sam_parse's) against the
    reference's record of each line, SEQ and QUAL through their offsets."""
    recs = parsed["records"]
    assert len(recs) == len(expected), (tag, len(recs), len(expected))
    for k, (r, e) in enumerate(zip(recs, expected)):
        seq_at, qual_at = int(r["line"]) + int(r["seq_off"]), int(r["line"]) + int(r["qual_off"])
        first = int(r["cigar"])
        got = dict(flag=int(r["flag"]), pos=int(r["pos"]), mapq=int(r["mapq"]), mate_same_contig=int(r["mate_same_contig"]),
                   seq=text[seq_at:seq_at + int(r["seq_len"])], qual=text[qual_at:qual_at + int(r["qual_len"])],
                   words=[int(w) for w in parsed["pool"][first:first + int(r["n_cigar"])]])
        assert got == e, (tag, k, got, e)


def parse_text(fixture, side):
    """Every line of the parse fixture that is no syntax error as one text, and the records expected of it."""
    exp = [(c, parse_expectation(c, side)) for c in fixture["parse"]]
    text = "\n".join(c["input"] for c, e in exp if e != "error").encode("latin-1")
    return text, [e for _, e in exp if isinstance(e, dict)], exp


def test_load_all_reads_equals_the_reference_line_by_line(fixture):
    text, expected, exp = parse_text(fixture, "restatement")
    assert len(expected) > 900 and sum(e == "skip" for _, e in exp) >= 20
    check_parsed_text(text, SR.load_all_reads(text), expected, "load_all_reads")
    for c, e in exp:
        if e == "error":
            with pytest.raises(SR.SamSyntax) as err:
                SR.load_all_reads("a 0 b 1 0 1M = 0 0 A I\n" + c["input"] + "\n")
            assert err.value.line_no == 2, c["name"]


# ---- the live form ---------------------------------------------------------------------

RANDOM = dict(parse=lambda: P.parse_random(9101), prepare=lambda: P.prepare_random(9102), align=lambda: P.align_random(9103),
              likelihoods=lambda: P.likelihood_random(9104), normalize=lambda: P.normalize_random(9105),
              genotype=lambda: P.genotype_random(9106), chain=lambda: P.chain_random(9107))


@pytest.mark.parametrize("stage", P.STAGES)
def test_restatement_equals_the_reference_live(reference, libs, stage):
    rows = [dict(name=name, input=x, output=P.reference_output(stage, reference, x)) for name, x in RANDOM[stage]()]
    assert any(not r["output"]["threw"] for r in rows)
    check_stage(stage, rows, libs)


def test_fixture_is_what_the_reference_gives_now(reference, fixture):
    """The committed outputs against the library built from the reference tree at hand."""
    for stage in P.STAGES:
        for case in fixture[stage]:
            now = P.encode(P.reference_output(stage, reference, case["input"]))
            assert now == P.encode(case["output"]), (stage, case["name"])
