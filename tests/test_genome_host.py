"""CPU: csrc/genome_body.hpp compiled for the host into a stand-alone program
(tests/cpp/genome_host_main.cpp) under -fsanitize=address,undefined, the text,
the name pool and the table in heap blocks of exactly their sizes: contig_of
per record and the contig of every window against the restatement
(genome_restate.py) on the fixture of genome_cases.py, for the table of twelve
names and for the table of 300. No GPU and no preloaded library."""
import os
import subprocess

import pytest

import genome_cases as GC
import genome_restate as GR
import sam_cases as SC
import sam_restate as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("genome_host") / "genome_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSAMX_HOST_ONLY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "genome_host_main.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, tmp_path, sam, contigs, region):
    fin, ftab, fout = tmp_path / "in.sam", tmp_path / "table.txt", tmp_path / "out.txt"
    fin.write_bytes(sam)
    ftab.write_text("".join(f"{n} {len(r)}\n" for n, r in contigs))
    p = subprocess.run([exe, str(fin), str(ftab), str(region), str(fout)], timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = fout.read_text().split("\n")
    n = int(rows[0].split()[1])
    recs = [tuple(int(x) for x in r.split()) for r in rows[1:1 + n]]
    nw = int(rows[1 + n].split()[1])
    wins = [int(x) for x in rows[2 + n:2 + n + nw]]
    return recs, wins, int(rows[2 + n + nw].split()[1])


def _extra_lines():
    """Names that are near misses of the table's: prefixes, extensions, another case, '*', 255 and 256 bytes."""
    near = ["chrT_al", "chrT_altx", "ch", "chrt", "*", "chrT2", "chr", GC.LONG_NAME[:-1], GC.LONG_NAME + "n",
            GC.LONG_NAME[:-1] + "m", "n" * 255, "x" * 300]
    return "".join(SC.line(qname="q" * (55 + k), rname=n, seq="ACGT") + "\n" for k, n in enumerate(near))


@pytest.mark.parametrize("table,region", [("twelve", 245), ("big", 245), ("twelve", 1), ("big", 7)])
def test_host_body_equals_restatement(exe, tmp_path, table, region):
    g = GC.genome()
    contigs = g["contigs"] if table == "twelve" else GC.big_table()
    sam = g["sam"] + _extra_lines().encode() + SC.line(qname="last_line_without_newline", rname="chrU").encode()
    recs, wins, past_first = _run(exe, tmp_path, sam, contigs, region)
    parsed = SR.load_all_reads(sam)
    want = GR.contig_of(sam, parsed["records"], [n for n, _ in contigs])
    assert [r[0] for r in recs] == [r["line"] for r in parsed["records"]]
    assert [r[1] for r in recs] == want
    assert want.count(-1) == 10 and set(want) == {-1} | {k for k, (n, _) in enumerate(contigs) if n in GC.ORDER and n != "chrEmpty"}
    exp = [c for c, (_, ref) in enumerate(contigs) for _ in range((len(ref) + region - 1) // region)]
    assert wins == exp and len(set(wins)) == len(contigs)
    if table == "big":
        assert past_first > 0      # some lookups probe past their first slot
