"""GPU: the C++ drop-in (include/hc_region.hpp, hc::MI355XRegionCaller) called
from a compiled C++ program with SAMRecord / Haplotype / Interval / Variant
stand-ins on seeded regions, against the three separate drop-ins in the same
program; every mismatch count it writes must be zero."""
import json
import os
import subprocess

import pytest

import hcphmm
import region_workloads as RW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_region_caller_dropin(tmp_path, engine):
    exe = tmp_path / "region_call"
    libdir = os.path.dirname(hcphmm.LIB_PATH)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "region_call.cpp"), "-L", libdir, "-lhcpairhmm",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    regs = RW.regions(8, RW.SEED + 1)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.json"
    RW.write_regions(fin, regs)
    done = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:], fout.read_text() if fout.exists() else "")
    out = json.loads(fout.read_text())
    assert out["regions"] == 8 and out["haplotypes"] == sum(len(r["haps"]) for r in regs)
    assert out["reads"] == sum(len(r["reads"]) for r in regs)
    assert 0 < out["reads_kept"] < out["reads"] and out["variants"] >= 4
    for k in ("sw_mismatch", "keep_mismatch", "variant_mismatch", "passed_in_cigar_mismatch"):
        assert out[k] == 0, out
