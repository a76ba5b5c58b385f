"""GPU: the C++ drop-in hc::MI355XIntervalCaller (include/hc_intervals.hpp) in a
compiled program (tests/cpp/intervals_dropin.cpp) on the twelve contigs of
genome_cases.py: a SAM file and a BAM file (told apart by their first two
bytes), intervals from a BED file and from the `intervals` member together. The
VCF equals the Python call's, with and without the file's index. Then the BED
errors with their line, an interval on a name that is no FASTA record, and an
index cut short."""
import os
import subprocess

import pytest

import bam_cases as BC
import genome_cases as GC
import hcintervals
import hcphmm
import intervals_cases as IC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BED = ("# panel\ntrack name=panel\nbrowser position chrT\n\nchrT\t300\t800\texon1\t0\t+\nchrU 151 152\n"
       "chrT\t700\t1000\n")
EXTRA = [("chrF", 8990, 9000), ("chrU", 150, 151)]


@pytest.fixture(scope="module")
def g():
    return GC.genome()


@pytest.fixture(scope="module")
def work(engine, g, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("intervals_dropin")
    exe = tmp / "intervals_dropin"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "intervals_dropin.cpp"), "-L", os.path.dirname(hcphmm.LIB_PATH),
                    "-lhcpairhmm", "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH), "-o", str(exe)], check=True)
    (tmp / "ref.fa").write_text("".join(f">{n}\n" + "".join(r.decode()[i:i + 60] + "\n" for i in range(0, len(r), 60))
                                        for n, r in g["contigs"]))
    f = IC.sorted_genome(4096)                 # sorted by position, with its index
    bam = f["bam"]
    (tmp / "reads.bam").write_bytes(bam)
    (tmp / "reads.bam.bai").write_bytes(f["bai"])
    (tmp / "reads.sam").write_bytes(BC.sam_of(bam))
    (tmp / "panel.bed").write_text(BED)
    return dict(tmp=tmp, exe=str(exe), bam=bam)


def _run(work, reads, out, bed="panel.bed", index="-", extra=EXTRA):
    tmp = work["tmp"]
    args = [work["exe"], str(tmp / reads), str(tmp / "ref.fa"), str(tmp / out), bed if bed == "-" else str(tmp / bed),
            index if index == "-" else str(tmp / index), "20261020"]
    for name, b, e in extra:
        args += [name, str(b), str(e)]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


def test_the_drop_in_writes_the_python_calls_vcf(work, g):
    names = [n for n, _ in g["contigs"]]
    intervals = hcintervals.parse_bed(BED, names) + IC.by_name(names, *EXTRA)
    e = hcintervals.call_genome_bam(work["bam"], g["contigs"], intervals, seed=20261020)
    assert e["vcf"].count(b"\n") > IC.HEADER_LINES + 1 and len({ln.split(b"\t")[0] for ln in e["vcf"].split(b"\n")[4:-1]}) >= 2
    for reads, out, index in (("reads.bam", "bam.vcf", "-"), ("reads.sam", "sam.vcf", "-"), ("reads.bam", "bai.vcf", "reads.bam.bai")):
        p = _run(work, reads, out, index=index)
        assert p.returncode == 0, p.stderr
        assert p.stdout.split() == ["contigs", "12", "windows", "76", "asked", str(len(e["asked"]))]
        assert (work["tmp"] / out).read_bytes() == e["vcf"], reads


def test_bed_and_interval_errors_name_their_line(work):
    tmp = work["tmp"]
    (tmp / "unknown.bed").write_text("chrT\t0\t10\n\nchrNone\t0\t10\n")
    (tmp / "short.bed").write_text("chrT\t0\n")
    (tmp / "word.bed").write_text("#\nchrT\tzero\t10\n")
    for bed, text in (("unknown.bed", "BED line 3: chrNone is no FASTA record"), ("short.bed", "BED line 1: fewer than three"),
                      ("word.bed", "BED line 2: begin or end is not a number")):
        p = _run(work, "reads.sam", "x.vcf", bed=bed)
        assert p.returncode == 3 and text in p.stderr, p.stderr
    p = _run(work, "reads.sam", "x.vcf", extra=[("chrNone", 0, 1)])
    assert p.returncode == 3 and "chrNone is no FASTA record" in p.stderr, p.stderr
    p = _run(work, "reads.bam", "x.vcf", extra=[("chrU", 0, 301)])
    assert p.returncode == 3 and "interval 3: end above the contig's ref_len" in p.stderr, p.stderr
    p = _run(work, "reads.sam", "x.vcf", bed="-", extra=[])
    # no interval at all: an empty vector's data() may be null, and the null is checked first
    assert p.returncode == 3 and p.stderr.strip() in ("hc_intervals: null intervals", "hc_intervals: n_intervals below 1"), p.stderr


def test_a_broken_index_is_invalid_input(work):
    (work["tmp"] / "cut.bai").write_bytes((work["tmp"] / "reads.bam.bai").read_bytes()[:50])
    p = _run(work, "reads.bam", "x.vcf", index="cut.bai")
    assert p.returncode == 3 and "BAI: cut short" in p.stderr, p.stderr
    p = _run(work, "reads.bam", "x.vcf", index="none.bai")
    assert p.returncode == 4 and "cannot open" in p.stderr, p.stderr
