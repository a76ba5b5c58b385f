"""CPU: the region caller's C ABI (include/hc_region.h) is exported and mirrored,
its headers compile, and the generator's committed seed makes a test set that
reaches the filter, the fp64 rescue and every site status (the reference chain
on the CPU says so)."""
import os
import subprocess

import numpy as np
import pytest

import hcphmm
import hcregion
import region_chain
import region_workloads as RW
from gt_restate import EMITTED, HOM_REF, LOW_QUALITY_HET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    hcphmm.ensure_built()
    return hcregion.lib()


def test_exports_and_mirrors_every_declared_region_symbol(built):
    syms = hcregion.declared_symbols()
    assert len(syms) == 6, syms
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [s for s in syms if s not in exported]
    assert "hcx_region_finish" in exported
    assert hcregion.mirrored_symbols() == syms


def test_region_structs_match_the_header(tmp_path):
    """sizeof / offsetof as the C compiler sees them against the ctypes mirror."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hc_region.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(hc_region_hap), sizeof(hc_region_in),\n'
                   '  offsetof(hc_region_in, haps), offsetof(hc_region_in, reads), offsetof(hc_region_in, read_begin),\n'
                   '  offsetof(hc_region_in, n_reads)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    import ctypes as C
    R = hcregion.RegionIn
    assert got == [C.sizeof(hcregion.Hap), C.sizeof(R), R.haps.offset, R.reads.offset, R.read_begin.offset,
                   R.n_reads.offset]


def test_region_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "hc_region.h"\nint main(void) { hc_region_calls* c = 0; '
                   'return hc_region_call(0, 0, HC_REGION_WANT_L | HC_REGION_F64, &c) == 12345; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_region_cpp_dropin_compiles(tmp_path):
    """include/hc_region.hpp against stand-in SAMRecord / Haplotype / Variant /
    Interval types shaped like the reference's."""
    src = tmp_path / "dropin.cpp"
    src.write_text(r'''
#include "hc_region.hpp"
#include <string>
#include <string_view>
#include <vector>
struct Interval { std::string contig; std::size_t begin, end; };
struct SAMRecord { std::string SEQ, QUAL; Interval iv;
  static inline const std::string GOP = std::string(200, 'I');
  static inline const std::string GCP = std::string(200, '+');
  auto insertionGOP() const { return std::string_view{GOP}.substr(0, SEQ.size()); }
  auto deletionGOP() const { return std::string_view{GOP}.substr(0, SEQ.size()); }
  auto overallGCP() const { return std::string_view{GCP}.substr(0, SEQ.size()); }
  Interval get_interval() const { return iv; } };
struct Cigar { std::string t; Cigar() = default; Cigar(std::string s) : t(std::move(s)) {}
  std::string to_string() const { return t; } };
struct Haplotype { std::string bases; std::size_t alignment_begin_wrt_ref = 0; Cigar cigar; };
struct Variant { Interval loc; std::vector<std::string> alleles; std::pair<std::size_t, std::size_t> gt; std::size_t gq;
  Variant(Interval l, std::vector<std::string> a, std::pair<std::size_t, std::size_t> g, std::size_t q)
    : loc(std::move(l)), alleles(std::move(a)), gt(g), gq(q) {} };
int main() {
  std::vector<Haplotype> h{{"ACGTACGT"}, {"ACGAACGT"}};
  std::vector<SAMRecord> r{{"ACGT", "IIII", {"chr", 10, 14}}};
  hc::MI355XRegionCaller<Variant> caller;
  try { auto v = caller.call(r, h, std::string_view{"ACGTACGT"}, Interval{"chr", 10, 18}, Interval{"chr", 12, 16});
        return int(v.size()) > 100; }
  catch (const std::exception&) { return 0; }
}
''')
    exe = tmp_path / "dropin"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", os.path.dirname(hcphmm.LIB_PATH), "-lhcpairhmm",
                    "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH), "-o", str(exe)], check=True)
    assert exe.exists()


def test_region_call_no_silent_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hcregion.RegionError) as e:
        hcregion.call_regions(RW.regions(1, RW.SEED))
    assert e.value.code == hcphmm.ENODEV


def test_generator_is_seeded_and_shaped():
    a, b = RW.regions(3, RW.SEED), RW.regions(3, RW.SEED)
    for x, y in zip(a, b):
        assert x["ref"] == y["ref"] and x["haps"] == y["haps"] and x["reads"] == y["reads"]
        assert np.array_equal(x["read_begin"], y["read_begin"]) and np.array_equal(x["read_end"], y["read_end"])
    for x in a:
        assert len(x["ref"]) == 415 and x["origin_end"] - x["origin_begin"] == 245
        assert 40 <= len(x["reads"]) <= 240 and 2 <= len(x["haps"]) <= 17
        assert x["haps"][0] == x["ref"]
        for (bases, q, i, d, c), rb, re_ in zip(x["reads"], x["read_begin"], x["read_end"]):
            assert 100 <= len(bases) <= 151 and len(q) == len(i) == len(d) == len(c) == len(bases)
            assert all(53 <= v <= 73 for v in q)
            assert x["padded_begin"] <= rb < re_ <= x["padded_begin"] + 415
    s = RW.sized(2, 415, 32)
    assert all(len(x["reads"]) == 415 and len(x["haps"]) == 32 for x in s)


def test_committed_seed_reaches_every_path(oracle_lib, sw_oracle_lib, gt_oracle_lib):
    """The reference chain on the CPU over the GPU tests' 24 regions: at least one
    filtered read, one fp64-rescued pair and one site of each status."""
    c = region_chain.cpu_chain(RW.regions(24, RW.SEED), oracle_lib, sw_oracle_lib, gt_oracle_lib)
    assert sum(int((~k).sum()) for k in c["keep"]) >= 1
    assert sum(int(k.sum()) for k in c["keep"]) >= 1
    assert c["rescued"] >= 1
    status = [s["status"] for s in c["sites"]]
    for want in (EMITTED, HOM_REF, LOW_QUALITY_HET):
        assert status.count(want) >= 1, (want, status)
