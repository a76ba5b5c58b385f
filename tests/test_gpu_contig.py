"""GPU: hc_contig_call (include/hc_contig.h) on the 13-window contig of
sam_cases.py, for two seeds and pick="first": window bounds, reference slices
and picked reads against the restatement (sam_restate.py); statuses, haplotype
counts, sites and surviving reads against hccall.call_windows on the
restatement's windows (the chain the parent commit has); the VCF text against
the restatement's print of those sites, byte for byte. Then batches of five
windows in a fresh process, unplaced and defective reads, and a reshuffled file."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hccall
import hccontig
import hcphmm
import sam_cases as SC
import sam_restate as SR
from gt_restate import EMITTED

pytestmark = pytest.mark.gpu

PICKS = [("seeded", 0), ("seeded", 20261020), ("first", 0)]
CALLED, NO_READS, NO_VARIATION = 0, 1, 2


@pytest.fixture(scope="module")
def contig():
    return SC.contig()


@pytest.fixture(scope="module")
def expected(engine, contig):
    """Per pick: the restatement's windows and the parent's chain on those with reads."""
    out = {}
    for pick, seed in PICKS:
        parsed, wins = SC.restated_windows(contig["sam"], contig["ref"], pick, seed)
        sent = [k for k, w in enumerate(wins) if w["picked"]]
        chain = hccall.call_windows([wins[k]["call"] for k in sent], want_site_reads=True)
        for k, c in zip(sent, chain["windows"]):
            wins[k]["chain"] = c
        sites = [dict(s, region=sent[s["region"]]) for s in chain["sites"]]
        out[(pick, seed)] = dict(parsed=parsed, windows=wins, sites=sites)
    return out


@pytest.fixture(scope="module")
def got(engine, contig):
    return {(pick, seed): hccontig.call_contig(contig["sam"], SC.CONTIG, contig["ref"], seed=seed, pick=pick,
                                               want_site_reads=True) for pick, seed in PICKS}


def test_the_set_reaches_every_ending(expected):
    """On the expected side, so that it cannot hide a failure."""
    for key, e in expected.items():
        status = [w["chain"]["status"] if "chain" in w else NO_READS for w in e["windows"]]
        assert len(status) == 13
        assert status[SC.NO_READS_WINDOW] == NO_READS and not e["windows"][SC.NO_READS_WINDOW]["picked"], key
        assert status[SC.NO_VARIANT_WINDOW] == NO_VARIATION, (key, status)
        emitted = {s["region"] for s in e["sites"] if s["status"] == EMITTED}
        assert len(emitted) >= 5 and all(status[w] == CALLED for w in emitted), (key, sorted(emitted), status)
    a, b, c = (expected[k] for k in PICKS)
    assert [w["picked"] for w in a["windows"]] != [w["picked"] for w in b["windows"]] != [w["picked"] for w in c["windows"]]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("key", PICKS)
def test_windows_equal_restatement_and_chain(got, expected, contig, key):
    g, e = got[key], expected[key]
    SC.assert_same_parse(dict(g["sam"], n_header_lines=e["parsed"]["n_header_lines"]), e["parsed"], "sam")
    assert len(g["windows"]) == len(e["windows"]) == 13
    for k, (a, b) in enumerate(zip(g["windows"], e["windows"])):
        for f in ("padded_begin", "padded_end", "origin_begin", "origin_end", "ref_len", "picked"):
            assert a[f] == b[f], (k, f, a[f], b[f])
        assert contig["ref"][a["padded_begin"]:a["padded_begin"] + a["ref_len"]] == b["call"]["ref"], k
        if "chain" in b:
            c = b["chain"]
            assert (a["status"], a["asm_status"], a["kmer_size"], a["n_haps"]) == \
                (c["status"], c["asm_status"], c["kmer_size"], len(c["haps"])), k
            assert a["reads"] == [b["picked"][j] for j in c["reads"]], k
        else:
            assert (a["status"], a["kmer_size"], a["n_haps"], a["reads"]) == (NO_READS, 0, 0, []), k
    assert len(g["sites"]) == len(e["sites"])
    for a, b in zip(g["sites"], e["sites"]):
        for f in ("region", "status", "begin", "loc_end", "n_alleles", "alleles", "n_keep", "keep_is_null",
                  "genotype_index", "a1", "a2", "genotype_quality"):
            assert a[f] == b[f], (f, a[f], b[f])
        assert a["hap_allele"].tolist() == b["hap_allele"].tolist() and a["keep"].tolist() == b["keep"].tolist()
        assert _bits(a["genotype_likelihoods"]) == _bits(b["genotype_likelihoods"])


@pytest.mark.parametrize("key", PICKS)
def test_vcf_equals_the_restatements_print(got, expected, key):
    text = SR.vcf(SC.CONTIG, expected[key]["sites"])
    assert text.count("\n") > 4 + 5
    assert got[key]["vcf"] == text.encode("latin-1")


_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import hccontig, hcphmm, sam_cases as SC
hcphmm.ensure_built(); hcphmm.init(0)
c = SC.contig()
out = []
for pick, seed in {picks!r}:
    r = hccontig.call_contig(c["sam"], SC.CONTIG, c["ref"], seed=seed, pick=pick)
    out.append(dict(vcf=r["vcf"].decode("latin-1"), windows=[[w[k] for k in ("picked", "status", "asm_status", "kmer_size",
               "n_haps", "reads")] for w in r["windows"]]))
print("RESULT " + json.dumps(out))
"""


def test_batches_of_five_windows_in_a_fresh_process(got):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HC_CONTIG_BATCH_WINDOWS="5")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=[here, os.path.dirname(hccontig.__file__)], picks=PICKS)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for key, r in zip(PICKS, res):
        g = got[key]
        assert r["vcf"].encode("latin-1") == g["vcf"], key
        assert r["windows"] == [[w[k] for k in ("picked", "status", "asm_status", "kmer_size", "n_haps", "reads")]
                                for w in g["windows"]], key


def _with_lines(contig, at, lines):
    """The contig's SAM text with `lines` inserted in front of 1-based line `at`."""
    rows = contig["sam"].decode().split("\n")
    return "\n".join(rows[:at - 1] + lines + rows[at - 1:]).encode()


def test_unplaced_read_fails_or_is_skipped(got, contig):
    n = len(contig["ref"])
    for at, pos in ((40, 0), (7, n + 1)):
        sam = _with_lines(contig, at, [SC.line(qname="unplaced", pos=pos, seq="A" * 60)])
        with pytest.raises(hccontig.ContigError) as e:
            hccontig.call_contig(sam, SC.CONTIG, contig["ref"])
        assert e.value.code == hcphmm.EINVAL and e.value.msg.startswith(f"line {at}: unplaced"), e.value.msg
        r = hccontig.call_contig(sam, SC.CONTIG, contig["ref"], skip_unplaced=True)
        assert r["vcf"] == got[("seeded", 0)]["vcf"]
    # the last position of the contig is a place (MAPQ 0: the chain drops the read, the pick does not)
    sam = _with_lines(contig, 40, [SC.line(qname="last", pos=n, mapq=0, seq="A" * 60)])
    r = hccontig.call_contig(sam, SC.CONTIG, contig["ref"])
    assert int(r["sam"]["records"]["pos"][r["windows"][12]["picked"][-1]]) == n
    # two unplaced reads: the lowest line is named
    sam = _with_lines(contig, 40, [SC.line(pos=0), SC.line(pos=0)])
    with pytest.raises(hccontig.ContigError) as e:
        hccontig.call_contig(sam, SC.CONTIG, contig["ref"])
    assert e.value.msg.startswith("line 40: ")


def _would_pick(sam, ref_len, line_no):
    """Per (pick, window): whether the record of 1-based line `line_no` is that window's pick at its position."""
    recs = SR.load_all_reads(sam)["records"]
    mine = next(k for k, r in enumerate(recs) if r["line_no"] == line_no)
    begin = recs[mine]["pos"] - 1
    bucket = [k for k, r in enumerate(recs) if r["pos"] - 1 == begin]          # file order
    out = {}
    for pick, seed in PICKS:
        for w, (pb, pe, _, _) in enumerate(SR.window_bounds(ref_len)):
            if pb <= begin < pe:
                out[(pick, seed, w)] = bucket[SR.pick_fn(pick, seed)(w, begin, len(bucket))] == mine
    return out


@pytest.mark.parametrize("defect,text", [(dict(cigar="*"), "n_cigar == 0"), (dict(cigar="59M"), "CIGAR's read length"),
                                         (dict(qual="I" * 59), "qual_len"),
                                         (dict(seq="A" * 65537), "seq_len above")])
def test_defective_read_fails_unless_a_flag_filter_hides_it(got, contig, defect, text):
    base = got[("seeded", 0)]
    # at a position that already holds reads, so that the defective one is picked or not by the seed
    recs = base["sam"]["records"]
    pos = next(int(recs["pos"][k]) for k in base["windows"][2]["picked"][10:]
               if (recs["pos"] == recs["pos"][k]).sum() >= 2)
    kw = dict(dict(qname="bad", pos=pos, seq="A" * 60), **defect)
    bad_sam = _with_lines(contig, 50, [SC.line(**kw)])
    would = _would_pick(bad_sam, len(contig["ref"]), 50)
    assert True in would.values() and False in would.values(), would     # picked by some of PICKS, not by others
    pick, seed, w = next(k for k, v in would.items() if v)
    for hidden in (dict(mapq=19), dict(flag=0x400), dict(flag=0x100), dict(rnext="chrOther")):
        r = hccontig.call_contig(_with_lines(contig, 50, [SC.line(**kw, **hidden)]), SC.CONTIG, contig["ref"], seed=seed,
                                 pick=pick)
        assert 50 in [int(r["sam"]["line_no"][k]) for k in r["windows"][w]["picked"]]   # picked there, and no failure
    for pick, seed in PICKS:
        with pytest.raises(hccontig.ContigError) as e:
            hccontig.call_contig(bad_sam, SC.CONTIG, contig["ref"], seed=seed, pick=pick)
        assert e.value.code == hcphmm.EINVAL and e.value.msg.startswith("line 50: ") and text in e.value.msg, e.value.msg
    # the engine is usable afterwards
    assert hccontig.call_contig(contig["sam"], SC.CONTIG, contig["ref"])["vcf"] == base["vcf"]


def test_scans_over_several_tiles(engine):
    """9 000 positions are three scan tiles of 4 096; with region 2 and padding 1
    the 4 500 windows are two. Picks and bounds against the restatement, the
    statuses against the chain on the restatement's windows."""
    c = SC.flat_contig()
    g = hccontig.call_contig(c["sam"], SC.CONTIG, c["ref"], seed=5)
    _, wins = SC.restated_windows(c["sam"], c["ref"], "seeded", 5)
    assert len(g["windows"]) == len(wins) == 37 and len(c["ref"]) > 2 * 4096
    assert [w["picked"] for w in g["windows"]] == [w["picked"] for w in wins]
    assert sum(len(w["picked"]) for w in wins) > 4096
    chain = hccall.call_windows([w["call"] for w in wins])
    assert [w["status"] for w in g["windows"]] == [w["status"] for w in chain["windows"]]
    assert len(g["sites"]) == len(chain["sites"])
    # every read behind the MAPQ filter: 4 500 windows of four bases end HC_CALL_NO_READS in the preparation
    g = hccontig.call_contig(c["sam_mapq0"], SC.CONTIG, c["ref"], region_size=2, padding_size=1, seed=5)
    _, wins = SC.restated_windows(c["sam_mapq0"], c["ref"], "seeded", 5, region=2, padding=1)
    assert len(g["windows"]) == len(wins) == 4500
    for a, b in zip(g["windows"], wins):
        assert (a["padded_begin"], a["padded_end"], a["ref_len"], a["picked"]) == \
            (b["padded_begin"], b["padded_end"], b["ref_len"], b["picked"])
        assert a["status"] == NO_READS and a["reads"] == []
    assert g["vcf"] == SR.VCF_HEADER.encode()


def test_reads_per_position_are_bounded(engine, contig):
    def sam(n):
        return (SC.HEADER + "".join(SC.line(qname=f"d{k}", pos=700, mapq=0, seq="A" * 20) + "\n" for k in range(n))).encode()
    r = hccontig.call_contig(sam(4096), SC.CONTIG, contig["ref"], pick="first")
    assert [w["picked"] for w in r["windows"]] == [[], [], [0], [0]] + [[]] * 9    # 699 lies in two padded intervals
    with pytest.raises(hccontig.ContigError) as e:
        hccontig.call_contig(sam(4097), SC.CONTIG, contig["ref"])
    assert e.value.code == hcphmm.EINVAL and "more than 4096 reads begin at position 700" in e.value.msg


def test_reshuffled_file_gives_the_same_vcf(got, contig):
    for pick, seed in PICKS:
        r = hccontig.call_contig(contig["sam_reshuffled"], SC.CONTIG, contig["ref"], seed=seed, pick=pick)
        assert r["vcf"] == got[(pick, seed)]["vcf"], (pick, seed)


def test_argument_errors(engine, contig):
    def rc(**kw):
        a = dict(sam=contig["sam"], contig=b"c", ref=contig["ref"], ref_len=len(contig["ref"]), region=245, padding=85,
                 pick=0, flags=2)
        a.update(kw)
        h = C.c_void_p()
        return hccontig.lib().hc_contig_call(a["sam"], len(a["sam"] or b""), a["contig"], a["ref"], a["ref_len"], a["region"],
                                             a["padding"], 0, a["pick"], a["flags"], C.byref(h))
    for bad in (dict(region=0), dict(padding=246), dict(padding=-1), dict(region=700, padding=162), dict(ref_len=0),
                dict(ref=None), dict(contig=None), dict(flags=4), dict(pick=2)):
        assert rc(**bad) == hcphmm.EINVAL, bad


def test_exports_and_mirrors_every_declared_symbol(engine):
    syms = hccontig.declared_symbols(hccontig.HEADER)
    assert syms == ["hc_contig_call", "hc_contig_result_free", "hc_contig_result_reads", "hc_contig_result_sam",
                    "hc_contig_result_sites", "hc_contig_result_vcf", "hc_contig_result_window"]
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [s for s in syms if s not in exported]
    assert [s for s in hccontig.mirrored_symbols() if s.startswith("hc_contig_")] == syms
