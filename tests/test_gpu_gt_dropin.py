"""GPU: the C++ drop-in (include/hc_gt.hpp, hc::MI355XGenotyper) called from a
compiled C++ program with SAMRecord / Haplotype / Interval / Variant stand-ins
on seeded regions; the printed variants must be the restatement's emitted set."""
import os
import subprocess

import pytest

import gt_restate as RS
import gt_workloads as G
import hcphmm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_genotyper_dropin(tmp_path, gt_oracle_lib):
    exe = tmp_path / "gt_dropin"
    libdir = os.path.dirname(hcphmm.LIB_PATH)
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "gt_dropin.cpp"), "-L", libdir, "-lhcpairhmm",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    regs = G.regions(8, 415, 245, (8, 32), (50, 120), seed=72)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.txt"
    G.write_regions(fin, regs)
    subprocess.run([str(exe), "run", str(fin), str(fout)], check=True, timeout=120)
    exp = [f"{r['region']} {r['begin']} {r['loc_end']} {b','.join(r['alleles']).decode()} "
           f"{r['a1']}/{r['a2']} {r['genotype_quality']}"
           for r in RS.call_regions(regs, gt_oracle_lib) if r["status"] == RS.EMITTED]
    assert len(exp) >= 4
    assert fout.read_text().splitlines() == exp
    # the host bookkeeping restated in the same program agrees on the counts
    host = subprocess.run([str(exe), "host", str(fin), "1"], check=True, capture_output=True, text=True).stdout.split()
    recs = RS.call_regions(regs, gt_oracle_lib)
    assert [int(x) for x in host[1:]] == [len(recs), sum(len(r["keep"]) for r in recs),
                                          sum(int(r["hap_allele"].sum()) for r in recs),
                                          sum(len(a) for r in recs for a in r["alleles"])]
