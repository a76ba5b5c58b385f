"""GPU: the C++ drop-in (include/hc_asm.hpp, hc::MI355XAssembler) called from a
compiled C++ program with SAMRecord / Haplotype / Cigar stand-ins on scenarios
(b), (c) and (f): bases, scores, offsets and CIGARs must equal hcasm + hcsw on
the same input, per region and batched."""
import os
import subprocess

import pytest

import asm_util as U
import hcasm
import hcphmm
import hcsw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_assembler_dropin(tmp_path, engine):
    exe = tmp_path / "asm_dropin"
    libdir = os.path.dirname(hcphmm.LIB_PATH)
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "asm_dropin.cpp"), "-L", libdir, "-lhcpairhmm",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    regs = [r for n, r, _ in U.scenarios() if n in "bcf"]
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    fin.write_text(U.emul_input(regs))
    subprocess.run([str(exe), str(fin), str(fout)], check=True, timeout=120)
    exp = []
    aligner = hcsw.SWAligner()
    for reg, res in zip(regs, hcasm.assemble(regs)):
        exp.append(f"R {res['status']} {res['kmer_size']} {len(res['haps'])}")
        aln = aligner.align_many(reg["ref"], [h[0] for h in res["haps"]])
        exp += [f"H {U.score_bits(score):016x} {bases.decode()} {begin} {cigar}"
                for (bases, score), (begin, cigar) in zip(res["haps"], aln)]
    assert sum(line.startswith("H") for line in exp) == 5          # 2 + 2 + 1 haplotypes
    assert any("D" in line.split()[-1] for line in exp if line.startswith("H"))   # (c)'s deletion
    assert fout.read_text().splitlines() == exp + exp
