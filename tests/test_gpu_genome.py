"""GPU: hc_genome_call (include/hc_genome.h) on the twelve contigs of
genome_cases.py, for two seeds and pick="first", against the stand-in rule of
the header: contig c's windows, picks, statuses, sites and surviving reads are
those of hccontig.call_contig (the parent commit's chain) on the text filtered
by RNAME, record indices translated; the VCF byte for byte. contig_of, the
contigs' window ranges and the picks also against the restatement
(genome_restate.py). Then batches of five windows in a fresh process, unplaced,
defective and too deep reads, argument errors, two identical runs and the
export list."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import genome_cases as GC
import genome_restate as GR
import hccontig
import hcgenome
import hcphmm
import sam_cases as SC
import sam_restate as SR
from gt_restate import EMITTED

pytestmark = pytest.mark.gpu

PICKS = [("seeded", 0), ("seeded", 20261020), ("first", 0)]
CALLED, NO_READS, NO_VARIATION = 0, 1, 2
WINDOW_FIELDS = ("contig", "padded_begin", "padded_end", "origin_begin", "origin_end", "ref_len", "picked", "status",
                 "asm_status", "kmer_size", "n_haps", "reads")
HEADER_LEN = len(SR.VCF_HEADER)


@pytest.fixture(scope="module")
def g():
    return GC.genome()


@pytest.fixture(scope="module")
def names(g):
    return [n for n, _ in g["contigs"]]


@pytest.fixture(scope="module")
def expected(engine, g):
    """Per pick: every contig's stand-in call, its windows, sites and VCF lines put one behind the other."""
    parts = [GR.filtered(g["sam"], name) for name, _ in g["contigs"]]
    out = {}
    for pick, seed in PICKS:
        wins, sites, vcf = [], [], SR.VCF_HEADER.encode()
        for c, ((name, ref), (text, index)) in enumerate(zip(g["contigs"], parts)):
            r = hccontig.call_contig(text, name, ref, seed=seed, pick=pick, want_site_reads=True)
            first = len(wins)
            for w in r["windows"]:
                wins.append(dict(w, contig=c, picked=[index[k] for k in w["picked"]], reads=[index[k] for k in w["reads"]]))
            sites += [dict(s, region=first + s["region"]) for s in r["sites"]]
            assert r["vcf"][:HEADER_LEN] == SR.VCF_HEADER.encode()
            vcf += r["vcf"][HEADER_LEN:]
        out[(pick, seed)] = dict(windows=wins, sites=sites, vcf=vcf)
    return out


@pytest.fixture(scope="module")
def got(engine, g):
    return {(pick, seed): hcgenome.call_genome(g["sam"], g["contigs"], seed=seed, pick=pick, want_site_reads=True)
            for pick, seed in PICKS}


@pytest.fixture(scope="module")
def restated(g):
    return {(pick, seed): GR.genome_windows(g["sam"], g["contigs"], pick, seed) for pick, seed in PICKS}


def test_the_set_reaches_every_ending(expected, names):
    """On the expected side, so that it cannot hide a failure."""
    for key, e in expected.items():
        status = [w["status"] for w in e["windows"]]
        assert len(status) == 76
        assert CALLED in status and NO_READS in status and NO_VARIATION in status, (key, status)
        on_t = [s for s in e["sites"] if s["status"] == EMITTED and e["windows"][s["region"]]["contig"] == names.index("chrT")]
        assert len(on_t) >= 5, key
        on_u = [s for s in e["sites"] if s["status"] == EMITTED and e["windows"][s["region"]]["contig"] == names.index("chrU")]
        assert [s["begin"] for s in on_u] == [GC.VARIANT_AT], key       # lines of a second contig in the VCF
        for name in GC.SHORT:
            assert any(w["picked"] for w in e["windows"] if w["contig"] == names.index(name)), (key, name)
        assert all(not w["picked"] and w["status"] == NO_READS for w in e["windows"] if w["contig"] == names.index("chrEmpty"))
    a, b, c = (expected[k] for k in PICKS)
    assert [w["picked"] for w in a["windows"]] != [w["picked"] for w in b["windows"]] != [w["picked"] for w in c["windows"]]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("key", PICKS)
def test_windows_and_sites_equal_the_stand_in(got, expected, key):
    a, e = got[key], expected[key]
    assert len(a["windows"]) == len(e["windows"]) == 76
    for k, (x, y) in enumerate(zip(a["windows"], e["windows"])):
        for f in WINDOW_FIELDS:
            assert x[f] == y[f], (k, f, x[f], y[f])
    assert len(a["sites"]) == len(e["sites"])
    for x, y in zip(a["sites"], e["sites"]):
        for f in ("region", "status", "begin", "loc_end", "n_alleles", "alleles", "n_keep", "keep_is_null",
                  "genotype_index", "a1", "a2", "genotype_quality"):
            assert x[f] == y[f], (f, x[f], y[f])
        assert x["hap_allele"].tolist() == y["hap_allele"].tolist() and x["keep"].tolist() == y["keep"].tolist()
        assert _bits(x["genotype_likelihoods"]) == _bits(y["genotype_likelihoods"])


@pytest.mark.parametrize("key", PICKS)
def test_vcf_equals_the_stand_ins_byte_for_byte(got, expected, names, key):
    assert expected[key]["vcf"].count(b"\n") > 4 + 5
    assert got[key]["vcf"] == expected[key]["vcf"]
    assert got[key]["vcf"] == GR.vcf(names, expected[key]["windows"], expected[key]["sites"]).encode("latin-1")
    chroms = [ln.split(b"\t")[0].decode() for ln in got[key]["vcf"].split(b"\n")[4:-1]]
    assert len(set(chroms)) >= 2 and [names.index(c) for c in chroms] == sorted(names.index(c) for c in chroms)


@pytest.mark.parametrize("key", PICKS)
def test_parse_contigs_and_picks_equal_the_restatement(got, restated, key):
    a, r = got[key], restated[key]
    SC.assert_same_parse(dict(a["sam"], n_header_lines=r["parsed"]["n_header_lines"]), r["parsed"], "sam")
    assert a["sam"]["contig_of"].tolist() == r["contig_of"]
    assert a["contigs"] == r["contigs"]
    for k, (x, y) in enumerate(zip(a["windows"], r["windows"])):
        for f in WINDOW_FIELDS[:7]:
            assert x[f] == y[f], (k, f, x[f], y[f])


def test_contig_of_with_300_names(got, restated, g):
    big = GC.big_table()
    a = hcgenome.call_genome(g["sam"], big, seed=0)
    where = {n: k for k, (n, _) in enumerate(big)}
    small = restated[("seeded", 0)]["contig_of"]
    assert a["sam"]["contig_of"].tolist() == [where[g["contigs"][c][0]] for c in small]
    assert a["sam"]["contig_of"].tolist() == GR.contig_of(g["sam"], restated[("seeded", 0)]["parsed"]["records"], list(where))
    assert len(a["contigs"]) == 300 and a["vcf"] == got[("seeded", 0)]["vcf"]


def test_one_contig_equals_the_contig_call(engine, g, names):
    ref = g["contigs"][names.index("chrT")][1]
    text, _ = GR.filtered(g["sam"], "chrT")
    a = hcgenome.call_genome(text, [("chrT", ref)], seed=3, skip_unplaced=True, want_site_reads=True)
    b = hccontig.call_contig(text, "chrT", ref, seed=3, skip_unplaced=True, want_site_reads=True)
    assert a["vcf"] == b["vcf"] and a["vcf"].count(b"\n") > 4 + 5
    assert [{k: v for k, v in w.items() if k != "contig"} for w in a["windows"]] == b["windows"]


_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import hcgenome, hcphmm, genome_cases as GC
hcphmm.ensure_built(); hcphmm.init(0)
g = GC.genome()
out = []
for pick, seed in {picks!r}:
    r = hcgenome.call_genome(g["sam"], g["contigs"], seed=seed, pick=pick)
    out.append(dict(vcf=r["vcf"].decode("latin-1"), windows=[[w[k] for k in ("picked", "status", "asm_status", "kmer_size",
               "n_haps", "reads")] for w in r["windows"]]))
print("RESULT " + json.dumps(out))
"""


def test_batches_of_five_windows_cross_contig_borders(got):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HC_CONTIG_BATCH_WINDOWS="5", HC_GENOME_TRACE="1")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=[here, os.path.dirname(hcgenome.__file__)], picks=PICKS)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    traces = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in p.stderr.splitlines() if ln.startswith("[hc_genome]")]
    assert len(traces) == len(PICKS)
    for key, r, tr in zip(PICKS, res, traces):
        a = got[key]
        assert r["vcf"].encode("latin-1") == a["vcf"], key
        assert r["windows"] == [[w[k] for k in ("picked", "status", "asm_status", "kmer_size", "n_haps", "reads")]
                                for w in a["windows"]], key
        sent = [w["contig"] for w in a["windows"] if w["picked"]]
        assert int(float(tr["sent"])) == len(sent)
        assert int(float(tr["chain_calls"])) == -(-len(sent) // 5)
        assert -(-len(sent) // 5) < sum(-(-sent.count(c) // 5) for c in set(sent))    # not a sum of per-contig ceilings


def _with_lines(sam, at, lines):
    """The text with `lines` inserted in front of 1-based line `at`."""
    rows = sam.decode().split("\n")
    return "\n".join(rows[:at - 1] + lines + rows[at - 1:]).encode()


def _fails(sam, contigs, **kw):
    with pytest.raises(hcgenome.GenomeError) as e:
        hcgenome.call_genome(sam, contigs, **kw)
    assert e.value.code == hcphmm.EINVAL
    return e.value.msg


def test_unplaced_read_fails_or_is_skipped(got, g, names):
    base = got[("seeded", 0)]["vcf"]
    n_alt = len(g["contigs"][names.index("chrT_alt")][1])
    long_unknown = "chrNowhere_" + "z" * 100
    cases = [(dict(rname="chrNone"), "RNAME chrNone is not"), (dict(rname="*"), "RNAME * is not"),
             (dict(rname=long_unknown), "RNAME " + long_unknown[:64] + " is not"),
             (dict(rname="chrT_al"), "RNAME chrT_al is not"), (dict(rname="chrT", pos=0), "POS 0 is 0 or past"),
             # past its own 40 bases, inside the sum of the lengths: it must not land on the next contig
             (dict(rname="chrT_alt", pos=n_alt + 1), f"POS {n_alt + 1} is 0 or past the {n_alt} bases of contig chrT_alt"),
             (dict(rname="chrT_alt", pos=n_alt + 30), "of contig chrT_alt")]
    for k, (kw, text) in enumerate(cases):
        at = 20 + 7 * k
        sam = _with_lines(g["sam"], at, [SC.line(qname="unplaced", seq="A" * 60, **kw)])
        msg = _fails(sam, g["contigs"])
        assert msg.startswith(f"line {at}: unplaced read, ") and text in msg, msg
        assert hcgenome.call_genome(sam, g["contigs"], skip_unplaced=True)["vcf"] == base, kw
    # the last position of a contig that is not the last is a place
    sam = _with_lines(g["sam"], 40, [SC.line(qname="last", rname="chrS65", pos=65, mapq=0, seq="A" * 60)])
    r = hcgenome.call_genome(sam, g["contigs"])
    w = r["windows"][r["contigs"][names.index("chrS65")]["first_window"]]
    k = w["picked"][-1]
    assert (int(r["sam"]["records"]["pos"][k]), int(r["sam"]["contig_of"][k]), w["ref_len"]) == (65, names.index("chrS65"), 65)
    # two offenders in different contigs: the lowest line is named, whatever its kind
    sam = _with_lines(g["sam"], 60, [SC.line(rname="chrNone"), SC.line(rname="chrU", cigar="3M")])
    assert _fails(_with_lines(sam, 30, [SC.line(rname="chr", pos=65)]), g["contigs"]).startswith("line 30: unplaced")
    assert _fails(sam, g["contigs"]).startswith("line 60: unplaced")
    sam = _with_lines(g["sam"], 60, [SC.line(rname="chrU", cigar="3M"), SC.line(rname="chrNone")])
    assert _fails(sam, g["contigs"]).startswith("line 60: a read that passes the flag filters has the CIGAR's")
    assert hcgenome.call_genome(g["sam"], g["contigs"])["vcf"] == base


def _would_pick(sam, contigs, c, line_no):
    """Per (pick, seed, contig-local window): whether the record of 1-based line `line_no` is that window's pick."""
    recs = SR.load_all_reads(sam)["records"]
    of = GR.contig_of(sam, recs, [n for n, _ in contigs])
    mine = next(k for k, r in enumerate(recs) if r["line_no"] == line_no)
    begin = recs[mine]["pos"] - 1
    bucket = [k for k, r in enumerate(recs) if of[k] == c and r["pos"] - 1 == begin]          # file order
    out = {}
    for pick, seed in PICKS:
        for w, (pb, pe, _, _) in enumerate(SR.window_bounds(len(contigs[c][1]))):
            if pb <= begin < pe:
                out[(pick, seed, w)] = bucket[SR.pick_fn(pick, seed)(w, begin, len(bucket))] == mine
    return out


@pytest.mark.parametrize("defect,text", [(dict(cigar="*"), "n_cigar == 0"), (dict(cigar="59M"), "CIGAR's read length"),
                                         (dict(qual="I" * 59), "qual_len"),
                                         (dict(seq="A" * 65537), "seq_len above")])
def test_defective_read_fails_unless_a_flag_filter_hides_it(got, g, names, defect, text):
    base = got[("seeded", 0)]
    c = names.index("chrT")
    assert c != 0
    first = base["contigs"][c]["first_window"]
    recs, of = base["sam"]["records"], base["sam"]["contig_of"]
    pos = next(int(recs["pos"][k]) for k in base["windows"][first + 2]["picked"][10:]
               if ((recs["pos"] == recs["pos"][k]) & (of == c)).sum() >= 2)
    kw = dict(dict(qname="bad", rname="chrT", pos=pos, seq="A" * 60), **defect)
    bad_sam = _with_lines(g["sam"], 50, [SC.line(**kw)])
    would = _would_pick(bad_sam, g["contigs"], c, 50)
    assert True in would.values() and False in would.values(), would     # picked by some of PICKS, not by others
    pick, seed, w = next(k for k, v in would.items() if v)
    for hidden in (dict(mapq=19), dict(flag=0x400), dict(flag=0x100), dict(rnext="chrOther")):
        r = hcgenome.call_genome(_with_lines(g["sam"], 50, [SC.line(**kw, **hidden)]), g["contigs"], seed=seed, pick=pick)
        assert 50 in [int(r["sam"]["line_no"][k]) for k in r["windows"][first + w]["picked"]]   # picked there, and no failure
    for pick, seed in PICKS:
        msg = _fails(bad_sam, g["contigs"], seed=seed, pick=pick)
        assert msg.startswith("line 50: ") and text in msg, msg
    # the engine is usable afterwards
    assert hcgenome.call_genome(g["sam"], g["contigs"])["vcf"] == base["vcf"]


def test_reads_per_position_are_bounded(got, g, names):
    def sam(n):
        return (SC.HEADER + "".join(SC.line(qname=f"d{k}", rname="chrU", pos=7, mapq=0, seq="A" * 20) + "\n"
                                    for k in range(n))).encode()
    r = hcgenome.call_genome(sam(4096), g["contigs"], pick="first")
    first = r["contigs"][names.index("chrU")]["first_window"]
    assert [w["picked"] for w in r["windows"]] == [[0] if k == first else [] for k in range(76)]
    msg = _fails(sam(4097), g["contigs"])
    assert "more than 4096 reads begin at position 7 (1-based) of contig chrU" in msg, msg
    assert hcgenome.call_genome(g["sam"], g["contigs"])["vcf"] == got[("seeded", 0)]["vcf"]


def test_argument_errors(engine, g):
    ref = g["contigs"][0][1]

    def rc(table, sam=g["sam"], n=None, region=245, padding=85, pick=0, flags=2 | 256):   # no read is placed: skipped
        arr = (hcgenome.Contig * max(len(table), 1))(*[hcgenome.Contig(nm, rf, ln) for nm, rf, ln in table])
        h = C.c_void_p()
        code = hcgenome.lib().hc_genome_call(sam, len(sam or b""), arr if table else None, len(table) if n is None else n,
                                             region, padding, 0, pick, flags, C.byref(h))
        msg = hcphmm.lib().hc_phmm_last_error().decode() if code else ""
        if not code:
            hcgenome.lib().hc_genome_result_free(h)
        return code, msg
    ok = [(b"a", ref, len(ref)), (b"b", ref, len(ref))]
    assert rc(ok)[0] == 0
    for bad in (dict(region=0), dict(padding=246), dict(padding=-1), dict(region=700, padding=162), dict(flags=4), dict(pick=2),
                dict(n=0), dict(n=-1)):
        assert rc(ok, **bad)[0] == hcphmm.EINVAL, bad
    assert rc([])[0] == hcphmm.EINVAL
    for entry in ((b"b", ref, 0), (b"b", None, 5), (None, ref, 5), (b"", ref, 5), (b"*", ref, 5), (b"b c", ref, 5),
                  (b"b\tc", ref, 5), (b"x" * 256, ref, 5)):
        code, msg = rc([ok[0], entry])
        assert code == hcphmm.EINVAL and "contig 1" in msg, (entry[0], msg)
    assert rc([ok[0], (b"x" * 255, ref, 5)])[0] == 0
    code, msg = rc([ok[0], ok[1], (b"c", ref, 5), (b"b", ref, 7)])
    assert code == hcphmm.EINVAL and "contigs 1 and 3 have the same name" in msg, msg
    # 2^31 windows in total: refused before any device work (the references are never read)
    code, msg = rc([(b"a", ref, 2 ** 30), (b"b", ref, 2 ** 30)], region=1, padding=0)
    assert code == hcphmm.EINVAL and "windows" in msg, msg


def test_two_runs_give_identical_bytes(got, g):
    a = got[("seeded", 20261020)]
    b = hcgenome.call_genome(g["sam"], g["contigs"], seed=20261020, pick="seeded", want_site_reads=True)
    assert a["vcf"] == b["vcf"] and a["windows"] == b["windows"] and a["contigs"] == b["contigs"]
    for k in ("records", "line_no", "pool", "contig_of"):
        assert a["sam"][k].tobytes() == b["sam"][k].tobytes(), k
    assert len(a["sites"]) == len(b["sites"])
    for x, y in zip(a["sites"], b["sites"]):
        for f in x:
            if isinstance(x[f], np.ndarray):
                assert x[f].tobytes() == y[f].tobytes(), f
            else:
                assert x[f] == y[f], f


def test_exports_and_mirrors_every_declared_symbol(engine):
    syms = hcgenome.declared_symbols()
    assert syms == ["hc_genome_call", "hc_genome_result_contig", "hc_genome_result_free", "hc_genome_result_reads",
                    "hc_genome_result_sam", "hc_genome_result_sites", "hc_genome_result_vcf", "hc_genome_result_window"]
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [s for s in syms if s not in exported]
    assert hcgenome.mirrored_symbols() == syms
