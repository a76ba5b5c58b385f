"""GPU: hc_genome_call_intervals (include/hc_intervals.h) on the twelve contigs of
genome_cases.py against the stand-in rule of the header. The expected side is
the plain call hcgenome.call_genome(..., skip_unplaced=True), filtered in Python
(intervals_cases.expected): never the code under test. Whole-contig intervals
for the three picks of test_gpu_genome.py with dense and sorted buckets, one
base at and beside chrU's variant, the window border of chrT, a contig without
reads, unsorted lists against their merged form, reads that are defective,
unplaced or too deep outside and inside the intervals, the argument errors, two
identical runs, the trace line and the export list."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import genome_cases as GC
import hcgenome
import hcintervals
import hcphmm
import intervals_cases as IC
import sam_cases as SC
from gt_restate import EMITTED

pytestmark = pytest.mark.gpu

PICKS = [("seeded", 0), ("seeded", 20261020), ("first", 0)]
KEYS = [(pick, seed, srt) for pick, seed in PICKS for srt in (False, True)]


@pytest.fixture(scope="module")
def g():
    return GC.genome()


@pytest.fixture(scope="module")
def names(g):
    return [n for n, _ in g["contigs"]]


@pytest.fixture(scope="module")
def plain(engine, g):
    """P of the stand-in rule, per pick."""
    return {(pick, seed): hcgenome.call_genome(g["sam"], g["contigs"], seed=seed, pick=pick, skip_unplaced=True,
                                               want_site_reads=True) for pick, seed in PICKS}


@pytest.fixture(scope="module")
def main_set(plain, names):
    """Intervals made from the plain call's own sites: chrU's variant, one emitted site of chrT, and one base beside
    another emitted site of chrT in another window."""
    p = plain[("seeded", 0)]
    t = names.index("chrT")
    on_t = [s for s in p["sites"] if s["status"] == EMITTED and p["windows"][s["region"]]["contig"] == t]
    first = on_t[0]
    other = next(s for s in on_t if s["region"] != first["region"] and s["begin"] + 1 < p["windows"][s["region"]]["origin_end"]
                 and s["begin"] + 1 not in [x["begin"] for x in on_t])
    return [(names.index("chrU"), GC.VARIANT_AT, GC.VARIANT_AT + 1), (t, first["begin"], first["begin"] + 1),
            (t, other["begin"] + 1, other["begin"] + 2)]


def _call(g, intervals, pick="seeded", seed=0, srt=False, sam=None, **kw):
    return hcintervals.call_genome(g["sam"] if sam is None else sam, g["contigs"], intervals, seed=seed, pick=pick,
                                   want_site_reads=True, sorted_buckets=srt, **kw)


def test_the_expected_side_keeps_and_drops_lines(plain, g, names, main_set):
    """On the plain call alone, so that the filter cannot hide a failure."""
    p = plain[("seeded", 0)]
    e = IC.expected(p, g["contigs"], main_set)
    kept = e["vcf"].split(b"\n")[IC.HEADER_LINES:-1]
    assert 1 <= len(kept) < len(p["vcf"].split(b"\n")[IC.HEADER_LINES:-1])          # a line in, a line out
    assert {ln.split(b"\t")[0] for ln in kept} == {b"chrT", b"chrU"}                 # lines of two contigs
    emitted = [s for s in e["sites"] if s["status"] == EMITTED]
    assert len(emitted) > len(kept)                                                  # a site in the sites, not in the text
    assert 0 < len(e["asked"]) < len(p["windows"])
    assert any(w["picked"] for k, w in enumerate(p["windows"]) if k not in e["asked"])
    # the interval beside chrU's variant, inside the same window
    u = names.index("chrU")
    b = IC.expected(p, g["contigs"], [(u, GC.VARIANT_AT + 1, GC.VARIANT_AT + 2)])
    assert [s["begin"] for s in b["sites"] if s["status"] == EMITTED] == [GC.VARIANT_AT]
    assert b["vcf"].count(b"\n") == IC.HEADER_LINES and b["asked"] == [p["contigs"][u]["first_window"]]


@pytest.mark.parametrize("key", KEYS)
def test_whole_contig_intervals_give_the_plain_calls_bytes(plain, g, key):
    pick, seed, srt = key
    p = plain[(pick, seed)]
    a = _call(g, IC.whole(g["contigs"]), pick, seed, srt)
    assert a["vcf"] == p["vcf"] and a["windows"] == p["windows"] and a["contigs"] == p["contigs"]
    assert a["asked"] == list(range(len(p["windows"])))
    assert a["merged"] == IC.whole(g["contigs"])
    IC.assert_sites(a["sites"], p["sites"])
    IC.assert_same_records(a, p)


@pytest.mark.parametrize("key", KEYS)
def test_the_main_set_equals_the_filtered_plain_call(plain, g, main_set, key):
    pick, seed, srt = key
    a = _call(g, main_set, pick, seed, srt)
    IC.assert_call(a, IC.expected(plain[(pick, seed)], g["contigs"], main_set), key)
    IC.assert_same_records(a, plain[(pick, seed)])       # the records out of scope stay, with their true contig_of


def test_one_base_at_the_variant_and_one_beside_it(plain, g, names):
    p = plain[("seeded", 0)]
    u = names.index("chrU")
    at = _call(g, [(u, GC.VARIANT_AT, GC.VARIANT_AT + 1)])
    IC.assert_call(at, IC.expected(p, g["contigs"], [(u, GC.VARIANT_AT, GC.VARIANT_AT + 1)]))
    assert at["vcf"].count(b"\n") == IC.HEADER_LINES + 1 and at["vcf"].split(b"\n")[-2].startswith(b"chrU\t151\t")
    for beside in (GC.VARIANT_AT - 1, GC.VARIANT_AT + 1):
        b = _call(g, [(u, beside, beside + 1)])
        IC.assert_call(b, IC.expected(p, g["contigs"], [(u, beside, beside + 1)]))
        assert b["vcf"].count(b"\n") == IC.HEADER_LINES
        assert [s["begin"] for s in b["sites"] if s["status"] == EMITTED] == [GC.VARIANT_AT]
        assert b["asked"] == at["asked"]


def test_the_window_border_of_chrT(plain, g, names):
    p = plain[("seeded", 20261020)]
    t = names.index("chrT")
    first = p["contigs"][t]["first_window"]
    for iv, asked in (([(t, 245, 246)], [first + 1]), ([(t, 244, 246)], [first, first + 1]), ([(t, 244, 245)], [first])):
        a = _call(g, iv, seed=20261020)
        assert a["asked"] == asked
        IC.assert_call(a, IC.expected(p, g["contigs"], iv), iv)
        assert all(a["windows"][w]["picked"] for w in asked)
        assert [w["status"] for k, w in enumerate(a["windows"]) if k not in asked] == [IC.NOT_ASKED] * (len(a["windows"]) - len(asked))


def test_a_contig_without_reads_is_asked_and_has_none(plain, g, names):
    e = names.index("chrEmpty")
    a = _call(g, [(e, 100, 400)])
    first = plain[("seeded", 0)]["contigs"][e]["first_window"]
    assert a["asked"] == [first, first + 1]
    assert [a["windows"][w]["status"] for w in a["asked"]] == [IC.NO_READS] * 2
    IC.assert_call(a, IC.expected(plain[("seeded", 0)], g["contigs"], [(e, 100, 400)]))
    assert not a["sites"] and a["vcf"].count(b"\n") == IC.HEADER_LINES


@pytest.mark.parametrize("srt", [False, True])
def test_an_unsorted_list_equals_its_merged_form(plain, g, names, srt):
    t, u, f = names.index("chrT"), names.index("chrU"), names.index("chrF")
    messy = [(u, 140, 160), (t, 500, 900), (f, 10, 20), (t, 100, 300), (t, 250, 600), (u, 140, 160), (t, 900, 1000),
             (f, 0, 10), (u, 150, 151), (t, 2000, 2001)]
    merged = [(f, 0, 20), (t, 100, 1000), (t, 2000, 2001), (u, 140, 160)]
    assert sorted(merged, key=lambda x: x[0]) == IC.IR.merge_sorted(messy) and (f < t < u)
    a, b = _call(g, messy, srt=srt), _call(g, merged, srt=srt)
    assert a["merged"] == b["merged"] == merged
    assert a["vcf"] == b["vcf"] and a["windows"] == b["windows"] and a["asked"] == b["asked"]
    IC.assert_sites(a["sites"], b["sites"])
    IC.assert_call(a, IC.expected(plain[("seeded", 0)], g["contigs"], messy), srt)


def _fails(call, *args, **kw):
    with pytest.raises(hcgenome.GenomeError) as e:
        call(*args, **kw)
    assert e.value.code == hcphmm.EINVAL
    return e.value.msg


@pytest.mark.parametrize("srt", [False, True])
def test_defective_and_unplaced_reads_out_of_scope_raise_nothing(plain, g, names, srt):
    t, u = names.index("chrT"), names.index("chrU")
    n_lines = g["sam"].count(b"\n")
    bad = (SC.line(qname="bad", rname="chrT", pos=1500, cigar="59M", seq="A" * 60) + "\n"
           + SC.line(qname="nowhere", rname="chrNone", seq="A" * 60) + "\n"
           + SC.line(qname="past", rname="chrU", pos=301, seq="A" * 60) + "\n").encode()
    sam = g["sam"] + bad                                   # behind every record: the record indices stay
    msg = _fails(hcgenome.call_genome, sam, g["contigs"], sorted_buckets=srt)
    assert msg.startswith(f"line {n_lines + 1}: a read that passes the flag filters has the CIGAR's"), msg
    far = [(u, 0, 300), (t, 0, 245)]
    a = _call(g, far, srt=srt, sam=sam)
    b = _call(g, far, srt=srt)
    IC.assert_call(a, b, contigs=False)
    IC.assert_call(a, IC.expected(plain[("seeded", 0)], g["contigs"], far), contigs=False)
    assert a["contigs"][t]["n_records"] == b["contigs"][t]["n_records"] + 1
    assert a["sam"]["contig_of"].tolist()[-3:] == [t, -1, u] and len(a["sam"]["line_no"]) == len(b["sam"]["line_no"]) + 3
    # an interval over the defective read, and one in window 5, whose padding [1140, 1555) holds position 1499
    for over in ([(t, 1499, 1500)], far + [(t, 1300, 1301)]):
        assert _fails(_call, g, over, srt=srt, sam=sam) == msg
    # the unplaced reads have no position an interval could cover
    assert _call(g, IC.whole(g["contigs"]), srt=srt, sam=g["sam"] + bad.split(b"\n", 1)[1])["vcf"] == plain[("seeded", 0)]["vcf"]
    assert _call(g, far, srt=srt)["vcf"] == b["vcf"]        # the engine is usable afterwards


@pytest.mark.parametrize("srt", [False, True])
def test_too_many_reads_at_a_position_out_of_scope_raise_nothing(plain, g, names, srt):
    f, u = names.index("chrF"), names.index("chrU")
    deep = "".join(SC.line(qname=f"d{k}", rname="chrF", pos=4950, mapq=0, seq="A" * 20) + "\n" for k in range(4097)).encode()
    sam = g["sam"] + deep
    msg = _fails(hcgenome.call_genome, sam, g["contigs"], sorted_buckets=srt)
    assert "more than 4096 reads begin at position 4950 (1-based) of contig chrF" in msg, msg
    far = [(u, 100, 200), (f, 0, 4000)]
    a = _call(g, far, srt=srt, sam=sam)
    IC.assert_call(a, _call(g, far, srt=srt), contigs=False)
    IC.assert_call(a, IC.expected(plain[("seeded", 0)], g["contigs"], far), contigs=False)
    assert _fails(_call, g, [(f, 4949, 4950)], srt=srt, sam=sam) == msg
    assert _fails(_call, g, far + [(f, 4700, 4701)], srt=srt, sam=sam) == msg      # window 19's padding [4570, 4985) holds 4949
    beyond = far + [(f, 5200, 5201)]                                               # window 21's [5060, 5475) does not
    IC.assert_call(_call(g, beyond, srt=srt, sam=sam), IC.expected(plain[("seeded", 0)], g["contigs"], beyond), contigs=False)


def _rc(g, intervals, n=None, null=False):
    p = hcintervals.Prepared(g["sam"], g["contigs"], intervals, skip_unplaced=True)
    h = C.c_void_p()
    code = hcintervals.lib().hc_genome_call_intervals(p.sam, len(p.sam), p.table, p.n, None if null else p.intervals,
                                                      len(intervals) if n is None else n, 245, 85, 0, 0, p.flags, C.byref(h))
    msg = hcphmm.lib().hc_phmm_last_error().decode() if code else ""
    if not code:
        p.free(h)
    return code, msg


@pytest.mark.parametrize("intervals,kw,text", [
    ([(0, 0, 1)], dict(null=True), "null intervals"),
    ([(0, 0, 1)], dict(n=0), "n_intervals below 1"),
    ([(0, 0, 1)], dict(n=-1), "n_intervals below 1"),
    ([(0, 0, 1), (-1, 0, 1)], {}, "interval 1: contig index outside the table"),
    ([(12, 0, 1)], {}, "interval 0: contig index outside the table"),
    ([(0, 0, 1), (1, 0, 1), (2, -1, 1)], {}, "interval 2: begin below 0"),
    ([(0, 5, 5)], {}, "interval 0: end not above begin"),
    ([(0, 6, 5)], {}, "interval 0: end not above begin"),
    ([(0, 0, 40), (0, 0, 41)], {}, "interval 1: end above the contig's ref_len"),
])
def test_argument_errors(engine, g, intervals, kw, text):
    assert len(g["contigs"]) == 12 and len(g["contigs"][0][1]) == 40
    assert _rc(g, [(0, 0, 40)]) == (0, "")
    code, msg = _rc(g, intervals, **kw)
    assert code == hcphmm.EINVAL and msg == text, msg
    assert _rc(g, [(0, 0, 40)]) == (0, "")


def test_the_plain_calls_arguments_are_still_checked(engine, g):
    assert "padding_size" in _fails(hcintervals.call_genome, g["sam"], g["contigs"], [(0, 0, 1)], padding_size=300)
    assert "same name" in _fails(hcintervals.call_genome, g["sam"], g["contigs"][:2] + g["contigs"][:1], [(0, 0, 1)])
    with pytest.raises(ValueError):
        hcintervals.call_genome(g["sam"], g["contigs"], [("chrNone", 0, 1)])


def test_a_plain_result_has_no_intervals(engine, g):
    p = hcgenome.Prepared(g["sam"], g["contigs"])
    h = p.run()
    try:
        out = hcintervals.results(h, [n.decode("latin-1") for n in p.names], windows=[])
        assert out["merged"] == [] and out["asked"] == []
    finally:
        p.free(h)


def test_two_runs_give_identical_bytes(g, main_set):
    a, b = (_call(g, main_set, seed=20261020, srt=True) for _ in range(2))
    assert a["vcf"] == b["vcf"] and a["windows"] == b["windows"] and a["asked"] == b["asked"] and a["merged"] == b["merged"]
    IC.assert_same_records(a, b)
    for x, y in zip(a["sites"], b["sites"]):
        for f in x:
            assert (x[f].tobytes() == y[f].tobytes()) if hasattr(x[f], "tobytes") else (x[f] == y[f]), f


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import genome_cases as GC, hcgenome, hcintervals, hcphmm
hcphmm.ensure_built(); hcphmm.init(0)
g = GC.genome()
r = hcintervals.call_genome(g["sam"], g["contigs"], [(11, 150, 151), (11, 150, 152), (4, 0, 245)], sorted_buckets={srt})
print("ASKED", len(r["asked"]), len(r["merged"]))
hcgenome.call_genome(g["sam"], g["contigs"])
"""


@pytest.mark.parametrize("srt", [False, True])
def test_the_trace_line_carries_the_new_keys(engine, srt):
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=[here, os.path.dirname(hcgenome.__file__)], srt=srt)],
                       env=dict(os.environ, HC_GENOME_TRACE="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in p.stderr.splitlines() if ln.startswith("[hc_genome]")]
    assert len(lines) == 2
    assert "ASKED 2 2" in p.stdout
    assert (lines[0]["intervals"], lines[0]["asked"], lines[0]["sorted"]) == ("2", "2", str(int(srt)))
    assert int(lines[0]["scoped"]) > 0 and "scope" in lines[0]
    assert list(lines[0]).index("resolve") < list(lines[0]).index("scope") < list(lines[0]).index("buckets")
    assert not {"intervals", "asked", "scoped", "scope"} & set(lines[1])            # the plain call's line is as it was


def test_exports_and_mirrors_every_declared_symbol(engine):
    syms = hcintervals.declared_symbols()
    assert syms == ["hc_bam_genome_call_intervals", "hc_bam_genome_result_index", "hc_genome_call_intervals",
                    "hc_genome_result_intervals"]
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [s for s in syms if s not in exported]
    assert hcintervals.mirrored_symbols() == syms
