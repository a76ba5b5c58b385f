"""GPU: the C++ drop-in hc::MI355XHaplotypeCaller (include/hc_contig.hpp),
compiled as tests/cpp/contig_dropin.cpp. The 13-window contig of sam_cases.py is
written as a SAM file and a FASTA file (50-column lines, a header comment,
lower-case stretches), do_work runs in a child process, and the file it writes
must equal, byte for byte, the restatement's print of the sites that
hccall.call_windows gives on the restatement's windows."""
import os
import subprocess

import pytest

import hccall
import hcphmm
import sam_cases as SC
import sam_restate as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("contig_dropin") / "contig_dropin"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "contig_dropin.cpp"),
                    "-L", os.path.dirname(hcphmm.LIB_PATH), "-lhcpairhmm",
                    "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH), "-o", str(out)], check=True)
    return str(out)


def _fasta(ref: bytes) -> str:
    """The first record is the contig; a second one must not be read."""
    seq = ref.decode()
    seq = seq[:300] + seq[300:900].lower() + seq[900:2000] + seq[2000:2100].lower() + seq[2100:]
    rows = [seq[k:k + 50] for k in range(0, len(seq), 50)]
    return f">{SC.CONTIG} a comment\twith white space\n" + "\n".join(rows) + "\n>chrOther\nACGTACGTAC\n"


def _expected_vcf(sam, ref, pick, seed):
    _, wins = SC.restated_windows(sam, ref, pick, seed)
    sent = [k for k, w in enumerate(wins) if w["picked"]]
    chain = hccall.call_windows([wins[k]["call"] for k in sent])
    return SR.vcf(SC.CONTIG, [dict(s, region=sent[s["region"]]) for s in chain["sites"]]).encode("latin-1")


@pytest.mark.parametrize("pick", ["seeded", "first"])
def test_do_work_writes_the_expected_file(engine, exe, tmp_path, pick):
    c = SC.contig()
    sam, fa, out = tmp_path / "reads.sam", tmp_path / "ref.fa", tmp_path / "out.vcf"
    sam.write_bytes(c["sam"])
    fa.write_text(_fasta(c["ref"]))
    p = subprocess.run([exe, str(sam), str(fa), str(out), str(SEED), pick], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.split() == ["windows", "13"]
    want = _expected_vcf(c["sam"], c["ref"], pick, SEED)
    assert want.count(b"\n") > 4 + 5
    assert out.read_bytes() == want


def test_errors_map_as_in_the_other_dropins(engine, exe, tmp_path):
    c = SC.contig()
    sam, fa, out = tmp_path / "reads.sam", tmp_path / "ref.fa", tmp_path / "out.vcf"
    fa.write_text(_fasta(c["ref"]))
    sam.write_bytes(c["sam"] + SC.line(pos=0).encode() + b"\n")
    n_lines = c["sam"].count(b"\n") + 1
    p = subprocess.run([exe, str(sam), str(fa), str(out), "0", "seeded"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 3 and f"line {n_lines}: unplaced" in p.stderr, p.stderr      # std::invalid_argument
    p = subprocess.run([exe, str(sam), str(fa), str(out), "0", "seeded", "skip"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and out.read_bytes() == _expected_vcf(c["sam"], c["ref"], "seeded", 0)
    p = subprocess.run([exe, str(tmp_path / "missing.sam"), str(fa), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 4 and "cannot open" in p.stderr                               # std::runtime_error
