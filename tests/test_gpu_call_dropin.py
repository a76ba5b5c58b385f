"""GPU: the C++ drop-ins hc::MI355XReadPrep (include/hc_prep.hpp) and
hc::MI355XWindowCaller (include/hc_call.hpp), compiled against stand-in
SAMRecord / Cigar / Haplotype / Interval / Variant types
(tests/cpp/call_region_dropin.cpp), on three windows of call_cases.py: a called
one with a deletion, one whose reads are all filtered and one without a
variant. The variants, the reads left in the vector and their SEQ, POS and CIGAR
text must equal what hccall / hcprep give on the same windows."""
import os
import subprocess

import pytest

import call_cases as CC
import hccall
import hcphmm
import hcprep
import prep_restate as PR
from gt_restate import EMITTED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICK = (1, 3, 4)


def build(tmp_path):
    exe = tmp_path / "call_region_dropin"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "call_region_dropin.cpp"),
                    "-L", os.path.dirname(hcphmm.LIB_PATH), "-lhcpairhmm",
                    "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH), "-o", str(exe)], check=True)
    return str(exe)


def program_input(wins) -> str:
    lines = [str(len(wins))]
    for w in wins:
        lines.append(f"{w['ref'].decode()} {w['padded_begin']} {w['padded_end']} {w['origin_begin']} {w['origin_end']} "
                     f"{len(w['reads'])}")
        for r in w["reads"]:
            lines.append(f"{r['flag']} {r['pos']} {r['mapq']} {r['cigar']} {'=' if r['mate_same'] else 'chr2'} "
                         f"{r['bases'].decode()} {r['quals'].decode()}")
    return "\n".join(lines) + "\n"


def _reads_after(w, records, indices):
    """POS, CIGAR text, SEQ, QUAL of the reads `indices` as the records rewrite them."""
    out = []
    for j in indices:
        r, p = w["reads"][j], records[j]
        cig = PR.parse_cigar(r["cigar"])
        if p["front_to_M"]:
            cig[0][1] = "M"
        if p["back_to_M"]:
            cig[-1][1] = "M"
        lo, hi = p["offset"], p["offset"] + p["length"]
        out.append(f"{p['new_pos']} {PR.cigar_text(cig)} {r['bases'][lo:hi].decode()} {r['quals'][lo:hi].decode()}")
    return out


def test_dropin_equals_the_python_mirrors(engine, tmp_path):
    wins = [CC.windows()[k] for k in PICK]
    exe = build(tmp_path)
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    fin.write_text(program_input(wins))
    subprocess.run([exe, str(fin), str(fout)], check=True, timeout=120)
    lines = iter(fout.read_text().splitlines())

    prep = hcprep.prep_reads([CC.prep_window(w) for w in wins])
    call = hccall.call_windows(wins, want_cigars=True)
    assert [w["status"] for w in call["windows"]] == [CC.CALLED, CC.NO_READS, CC.NO_VARIATION]
    n_emitted = 0
    for k, w in enumerate(wins):
        tag, wk, n = next(lines).split()
        assert (tag, int(wk)) == ("P", k)
        assert [next(lines) for _ in range(int(n))] == _reads_after(w, prep[k]["records"], prep[k]["kept"]), k
        g = call["windows"][k]
        tag, wk, status, nv, nr, nh = next(lines).split()
        assert (tag, int(wk), int(status)) == ("C", k, g["status"])
        sites = [s for s in call["sites"] if s["region"] == k and s["status"] == EMITTED]
        n_emitted += len(sites)
        assert int(nv) == len(sites)
        for s in sites:
            alleles = " ".join(a.decode() for a in s["alleles"])
            assert next(lines) == f"V {s['begin']} {s['loc_end']} {s['a1']} {s['a2']} {s['genotype_quality']} {alleles}"
        assert [next(lines) for _ in range(int(nr))] == _reads_after(w, g["prep"]["records"], g["reads"]), k
        assert int(nh) == len(g["haps"])
        for (bases, _), (begin, cigar) in zip(g["haps"], g["alignments"]):
            assert next(lines) == (f"H {begin} {cigar} {bases.decode()}" if cigar else f"H 0 * {bases.decode()}")
    assert n_emitted >= 1
    for k in range(len(wins)):
        g = call["windows"][k]
        sites = [s for s in call["sites"] if s["region"] == k and s["status"] == EMITTED]
        assert next(lines) == f"M {k} {g['status']} {len(sites)} {len(g['reads'])}"
    assert next(lines, None) is None
