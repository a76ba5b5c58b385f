"""GPU: the C++ drop-in hc::MI355XGenomeCaller (include/hc_genome.hpp), compiled
as tests/cpp/genome_dropin.cpp. The twelve contigs of genome_cases.py are
written as one FASTA file (50-column lines, a header comment, lower-case
stretches) and the reads as a SAM file; do_work runs in a child process, and
the file it writes must equal, byte for byte, the VCF of the Python call
(hcgenome.call_genome) on what hcgenome.read_fasta reads from the same file.
A FASTA file with two header lines in a row is refused."""
import os
import subprocess

import pytest

import genome_cases as GC
import genome_restate as GR
import hcgenome
import hcphmm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("genome_dropin") / "genome_dropin"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "genome_dropin.cpp"),
                    "-L", os.path.dirname(hcphmm.LIB_PATH), "-lhcpairhmm",
                    "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH), "-o", str(out)], check=True)
    return str(out)


def _fasta(contigs) -> str:
    out = ""
    for k, (name, ref) in enumerate(contigs):
        seq = ref.decode()
        seq = seq[:20] + seq[20:300].lower() + seq[300:2000] + seq[2000:2100].lower() + seq[2100:]
        out += f">{name}" + (" a comment\twith white space", "\tx", "")[k % 3] + "\n"
        out += "".join(seq[i:i + 50] + "\n" for i in range(0, len(seq), 50))
    return out


@pytest.mark.parametrize("pick", ["seeded", "first"])
def test_do_work_writes_the_python_calls_vcf(engine, exe, tmp_path, pick):
    g = GC.genome()
    sam, fa, out = tmp_path / "reads.sam", tmp_path / "ref.fa", tmp_path / "out.vcf"
    sam.write_bytes(g["sam"])
    fa.write_text(_fasta(g["contigs"]))
    table = hcgenome.read_fasta(fa.read_bytes())
    assert table == [(n, r.decode()) for n, r in g["contigs"]] == GR.read_fasta(fa.read_text())
    p = subprocess.run([exe, str(sam), str(fa), str(out), str(SEED), pick], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.split() == ["contigs", "12", "windows", "76"]
    want = hcgenome.call_genome(g["sam"], table, seed=SEED, pick=pick)["vcf"]
    assert want.count(b"\n") > 4 + 5 and len({ln.split(b"\t")[0] for ln in want.split(b"\n")[4:-1]}) >= 2
    assert out.read_bytes() == want


def test_errors_map_as_in_the_other_dropins(engine, exe, tmp_path):
    g = GC.genome()
    sam, fa, out = tmp_path / "reads.sam", tmp_path / "ref.fa", tmp_path / "out.vcf"
    sam.write_bytes(g["sam"])
    fa.write_text(_fasta(g["contigs"][:5]))
    p = subprocess.run([exe, str(sam), str(fa), str(out), "0", "seeded"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 3 and "unplaced read, RNAME" in p.stderr, p.stderr                      # std::invalid_argument
    p = subprocess.run([exe, str(sam), str(fa), str(out), "0", "seeded", "skip"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split()[:2] == ["contigs", "5"], p.stderr
    assert out.read_bytes() == hcgenome.call_genome(g["sam"], g["contigs"][:5], skip_unplaced=True)["vcf"]
    for bad in (">a\n>b\nACGT\n", ">a\nACGT\n>b\n", ">a"):
        fa.write_text(bad)
        p = subprocess.run([exe, str(sam), str(fa), str(out)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 3 and "has no sequence line" in p.stderr, (bad, p.stderr)
        with pytest.raises(ValueError):
            hcgenome.read_fasta(bad)
    fa.write_text(_fasta(g["contigs"]))
    p = subprocess.run([exe, str(tmp_path / "missing.sam"), str(fa), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 4 and "cannot open" in p.stderr                                        # std::runtime_error
