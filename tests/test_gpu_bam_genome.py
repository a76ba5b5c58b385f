"""GPU: hc_bam_genome_call (include/hc_bam.h) against its stand-in rule on the
twelve contigs of genome_cases.py: for the three picks of test_gpu_genome.py,
with dense and with sorted buckets, hcbam.call_genome_bam(to_bam(sam), contigs)
equals hcgenome.call_genome(sam_of(bam), contigs) in every window field, every
site field and likelihood bit, the records (but line, seq_off, qual_off and
line_no), contig_of and the VCF byte for byte. The BAM header lists the
references in the reverse of the caller's table order. Then a shuffled table, a
table that misses a reference with and without HC_CONTIG_SKIP_UNPLACED, two
identical runs, the C++ drop-in hc::MI355XBamGenomeCaller against
hc::MI355XGenomeCaller in compiled programs, the trace line and the export list."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_cases as BC
import genome_cases as GC
import hcbam
import hcgenome
import hcphmm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICKS = [("seeded", 0), ("seeded", 20261020), ("first", 0)]
KEYS = [(pick, seed, srt) for pick, seed in PICKS for srt in (False, True)]
WINDOW_FIELDS = ("contig", "padded_begin", "padded_end", "origin_begin", "origin_end", "ref_len", "picked", "status",
                 "asm_status", "kmer_size", "n_haps", "reads")
SITE_FIELDS = ("region", "status", "begin", "loc_end", "n_alleles", "alleles", "n_keep", "keep_is_null", "genotype_index",
               "a1", "a2", "genotype_quality")
RECORD_FIELDS = ("seq_len", "qual_len", "pos", "cigar", "n_cigar", "flag", "mapq", "mate_same_contig", "defect")


@pytest.fixture(scope="module")
def g():
    return GC.genome()


@pytest.fixture(scope="module")
def bam(g):
    refs = [(n, len(r)) for n, r in reversed(g["contigs"])]
    return BC.to_bam(g["sam"], refs, member_size=65280)


@pytest.fixture(scope="module")
def text(bam):
    return BC.sam_of(bam)


@pytest.fixture(scope="module")
def expected(engine, g, text):
    return {(pick, seed, srt): hcgenome.call_genome(text, g["contigs"], seed=seed, pick=pick, want_site_reads=True,
                                                    sorted_buckets=srt) for pick, seed, srt in KEYS}


@pytest.fixture(scope="module")
def got(engine, g, bam):
    return {(pick, seed, srt): hcbam.call_genome_bam(bam, g["contigs"], seed=seed, pick=pick, want_site_reads=True,
                                                     sorted_buckets=srt) for pick, seed, srt in KEYS}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


def _assert_same_call(a, e, t):
    assert len(a["windows"]) == len(e["windows"])
    for k, (x, y) in enumerate(zip(a["windows"], e["windows"])):
        for f in WINDOW_FIELDS:
            assert x[f] == y[f], (k, f, x[f], y[f])
    assert len(a["sites"]) == len(e["sites"])
    for x, y in zip(a["sites"], e["sites"]):
        for f in SITE_FIELDS:
            assert x[f] == y[f], (f, x[f], y[f])
        assert x["hap_allele"].tolist() == y["hap_allele"].tolist() and x["keep"].tolist() == y["keep"].tolist()
        assert _bits(x["genotype_likelihoods"]) == _bits(y["genotype_likelihoods"])
    assert a["vcf"] == e["vcf"]
    assert a["contigs"] == e["contigs"]
    ra, re_ = a["sam"]["records"], e["sam"]["records"]
    assert len(ra) == len(re_)
    for f in RECORD_FIELDS:
        assert ra[f].tolist() == re_[f].tolist(), f
    assert a["sam"]["pool"].tolist() == e["sam"]["pool"].tolist()
    assert a["sam"]["contig_of"].tolist() == e["sam"]["contig_of"].tolist()
    assert a["sam"]["line_no"].tolist() == list(range(1, len(ra) + 1))
    for k in (0, len(ra) // 2, len(ra) - 1):
        assert hcbam.hccontig.seq(a["bases"], ra[k]) == hcbam.hccontig.seq(t, re_[k])
        assert hcbam.hccontig.qual(a["bases"], ra[k]) == hcbam.hccontig.qual(t, re_[k])


def test_the_expected_side_has_lines_on_two_contigs(expected, text, g):
    assert text.count(b"\n") == g["sam"].count(b"\n")
    for key, e in expected.items():
        assert e["vcf"].count(b"\n") > 4 + 5, key
        chroms = {ln.split(b"\t")[0] for ln in e["vcf"].split(b"\n")[4:-1]}
        assert len(chroms) >= 2, key
    a, b, c = (expected[(p, s, False)] for p, s in PICKS)
    assert [w["picked"] for w in a["windows"]] != [w["picked"] for w in b["windows"]] != [w["picked"] for w in c["windows"]]


@pytest.mark.parametrize("key", KEYS)
def test_bam_call_equals_the_sam_call_on_the_canonical_text(got, expected, text, key):
    _assert_same_call(got[key], expected[key], text)


def test_small_members_and_a_shuffled_table(g, bam, text, expected):
    small = BC.to_bam(g["sam"], [(n, len(r)) for n, r in reversed(g["contigs"])], member_size=4096, level=1)
    assert BC.sam_of(small) == text
    _assert_same_call(hcbam.call_genome_bam(small, g["contigs"], want_site_reads=True), expected[("seeded", 0, False)], text)
    order = [5, 0, 11, 3, 7, 1, 9, 2, 10, 4, 8, 6]
    table = [g["contigs"][k] for k in order]
    a = hcbam.call_genome_bam(bam, table, seed=7, want_site_reads=True)
    _assert_same_call(a, hcgenome.call_genome(text, table, seed=7, want_site_reads=True), text)
    assert [c["name"] for c in a["contigs"]] == [n for n, _ in table]


def test_a_table_that_misses_a_reference(g, bam, text):
    table = [c for c in g["contigs"] if c[0] != "chrU"]
    with pytest.raises(hcbam.BamError) as e:
        hcbam.call_genome_bam(bam, table)
    assert e.value.code == hcphmm.EINVAL
    first = next(k for k, ln in enumerate(text.split(b"\n")[3:]) if ln.split(b"\t")[2] == b"chrU") + 1
    assert e.value.msg == f"record {first}: unplaced read, RNAME chrU is not in the contig table", e.value.msg
    with pytest.raises(hcgenome.GenomeError) as s:
        hcgenome.call_genome(text, table)
    assert s.value.msg == f"line {first + 3}: unplaced read, RNAME chrU is not in the contig table"
    a = hcbam.call_genome_bam(bam, table, skip_unplaced=True, want_site_reads=True)
    _assert_same_call(a, hcgenome.call_genome(text, table, skip_unplaced=True, want_site_reads=True), text)
    assert (a["sam"]["contig_of"] == -1).sum() > 50
    # refID -1 is unplaced too, and the engine is usable after the failure
    lines = text.split(b"\n")
    f = lines[10].split(b"\t")
    f[2], f[6] = b"*", b"*"
    star = b"\n".join(lines[:10] + [b"\t".join(f)] + lines[11:])
    with pytest.raises(hcbam.BamError) as e:
        hcbam.call_genome_bam(BC.to_bam(star, [(n, len(r)) for n, r in g["contigs"]]), g["contigs"])
    assert e.value.msg == "record 8: unplaced read, RNAME * is not in the contig table", e.value.msg


def test_two_runs_give_identical_bytes(got, g, bam):
    a = got[("seeded", 20261020, True)]
    b = hcbam.call_genome_bam(bam, g["contigs"], seed=20261020, pick="seeded", want_site_reads=True, sorted_buckets=True)
    assert a["vcf"] == b["vcf"] and a["windows"] == b["windows"] and a["contigs"] == b["contigs"] and a["bases"] == b["bases"]
    for k in ("records", "line_no", "pool", "contig_of"):
        assert a["sam"][k].tobytes() == b["sam"][k].tobytes(), k
    for x, y in zip(a["sites"], b["sites"]):
        for f in x:
            if isinstance(x[f], np.ndarray):
                assert x[f].tobytes() == y[f].tobytes(), f
            else:
                assert x[f] == y[f], f


def _build(tmp, name):
    out = tmp / name
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L", os.path.dirname(hcphmm.LIB_PATH), "-lhcpairhmm",
                    "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH), "-o", str(out)], check=True)
    return str(out)


def test_the_cpp_drop_in_writes_the_sam_drop_ins_vcf(engine, g, bam, text, tmp_path):
    exe_bam, exe_sam = _build(tmp_path, "bam_genome_dropin"), _build(tmp_path, "genome_dropin")
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(f">{n}\n" + "".join(r.decode()[i:i + 60] + "\n" for i in range(0, len(r), 60)) for n, r in g["contigs"]))
    (tmp_path / "reads.bam").write_bytes(bam)
    (tmp_path / "reads.sam").write_bytes(text)
    for exe, reads, out in ((exe_bam, "reads.bam", "bam.vcf"), (exe_sam, "reads.sam", "sam.vcf")):
        p = subprocess.run([exe, str(tmp_path / reads), str(fa), str(tmp_path / out), "20261020", "seeded"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert p.stdout.split() == ["contigs", "12", "windows", "76"]
    vcf = (tmp_path / "bam.vcf").read_bytes()
    assert vcf == (tmp_path / "sam.vcf").read_bytes() and vcf.count(b"\n") > 4 + 5
    (tmp_path / "raw.bam").write_bytes(BC.inflate(bam))
    p = subprocess.run([exe_bam, str(tmp_path / "raw.bam"), str(fa), str(tmp_path / "x.vcf")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 3 and "not a BGZF member" in p.stderr, p.stderr


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import bam_cases as BC, genome_cases as GC, hcbam, hcgenome, hcphmm
hcphmm.ensure_built(); hcphmm.init(0)
g = GC.genome()
bam = BC.to_bam(g["sam"], [(n, len(r)) for n, r in g["contigs"]])
hcbam.call_genome_bam(bam, g["contigs"])
hcgenome.call_genome(g["sam"], g["contigs"])
"""


def test_the_trace_names_the_front_and_its_phases(engine):
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=[here, os.path.dirname(hcbam.__file__)])],
                       env=dict(os.environ, HC_GENOME_TRACE="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith("[hc_genome]")]
    assert len(lines) == 2
    keys = [[kv.split("=")[0] for kv in ln.split()[1:]] for ln in lines]
    assert "front=bam" in lines[0].split() and "front=bam" not in lines[1]
    for phase in ("upload", "inflate", "crc", "frame", "decode", "readback", "resolve", "buckets", "picks", "vcf"):
        assert phase in keys[0], phase
    assert keys[1][:4] == ["parse", "resolve", "buckets", "picks"] and "inflate" not in keys[1]


def test_exports_and_mirrors_every_declared_symbol(engine):
    syms = hcbam.declared_symbols()
    assert syms == ["hc_bam_genome_call", "hc_bam_genome_result_bases", "hc_bam_parse", "hc_bam_result_bases",
                    "hc_bam_result_free", "hc_bam_result_header", "hc_bam_result_records", "hc_bam_result_reference",
                    "hc_bgzf_inflate", "hc_bgzf_result_bytes", "hc_bgzf_result_free", "hc_bgzf_result_members"]
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [s for s in syms if s not in exported]
    assert hcbam.mirrored_symbols() == syms
