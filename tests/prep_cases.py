"""Inputs shared by the read preparation's tests (test_prep_host.py,
test_gpu_prep.py): the grid, the compaction windows, the expected side from the
restatement (computed once) and the text format of tests/cpp/prep_host_main.cpp."""
from __future__ import annotations

import functools
import os
import subprocess

import prep_restate as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = "MIDNSHP=X"

# CIGAR shapes nM, aSbM, aMbS, aSbMcS, nS, aMbIcM, aMbDcM, aHbM; every one reads 40 bases
SHAPES = ["40M", "8S32M", "32M8S", "6S28M6S", "40S", "15M5I20M", "20M7D20M", "5H40M"]
SEQ_LEN = 40
WIN = (1000, 1400)
# 0-based begins: before the window's begin by more than, exactly and less than the
# read's length; inside; across the end by less than (down to 10 and 9 bases left),
# exactly and more than what is left of the read
BEGINS = [939, 959, 960, 969, 970, 971, 985, 1100, 1360, 1370, 1390, 1391, 1400, 1410, 1447]
FILTERS = [dict(), dict(mapq=19), dict(flag=0x400), dict(flag=0x100), dict(mate_same=0),
           dict(mapq=0, flag=0x500, mate_same=0), dict(flag=0x100, mate_same=0)]


def read(cigar, begin, reverse=False, seq_len=SEQ_LEN, mapq=60, flag=0, mate_same=1):
    return dict(flag=flag | (0x10 if reverse else 0), mapq=mapq, pos=begin + 1, cigar=cigar, mate_same=mate_same,
                seq_len=seq_len)


@functools.lru_cache(maxsize=None)
def grid():
    """One window per filter setting with shapes x strands x begins, and one
    window at the contig's start with front_length <, == and > alignment_begin."""
    wins = []
    for f in FILTERS:
        reads = [read(c, b, rev, **f) for c in SHAPES for rev in (False, True) for b in BEGINS]
        wins.append(dict(begin=WIN[0], end=WIN[1], reads=reads))
    low = []
    for c, fl in (("8S32M", 8), ("6S28M6S", 6), ("40S", 40)):
        for rev in (False, True):
            low += [read(c, b, rev) for b in (0, fl - 1, fl, fl + 1)]
    wins.append(dict(begin=0, end=400, reads=low))
    wins.append(dict(begin=5, end=30, reads=low))     # the same reads clipped on both sides
    return wins


def _kept(j):
    return read(f"{20 + j % 30}M", 1100 + j % 7, j % 2 == 1, seq_len=20 + j % 30)


def _dropped(j):
    return [read("40M", 1100, mapq=3), read("40M", 1100, flag=0x400), read("40M", 1100, flag=0x100),
            read("40M", 1100, mate_same=0), read("40M", 1395)][j % 5]


@functools.lru_cache(maxsize=None)
def compaction():
    """Windows of 0, 1, 63, 64, 65, 128 and 129 reads: none, all and every other
    read kept (both phases), and windows whose only kept read is read 64."""
    wins = []
    for n in (0, 1, 63, 64, 65, 128, 129):
        for pattern in ("none", "all", "even", "odd"):
            keep = dict(none=lambda j: False, all=lambda j: True, even=lambda j: j % 2 == 0, odd=lambda j: j % 2 == 1)[pattern]
            wins.append(dict(begin=WIN[0], end=WIN[1], reads=[_kept(j) if keep(j) else _dropped(j) for j in range(n)]))
    for n in (65, 128, 129):
        wins.append(dict(begin=WIN[0], end=WIN[1], reads=[_kept(j) if j == 64 else _dropped(j) for j in range(n)]))
    return wins


@functools.lru_cache(maxsize=None)
def expected(which: str):
    """The restatement's records of grid() or compaction(), computed once."""
    return [PR.records(w) for w in dict(grid=grid, compaction=compaction)[which]()]


def assert_same(got, exp, tag=""):
    """Every record field and the window totals."""
    assert len(got) == len(exp), tag
    for w, (g, e) in enumerate(zip(got, exp)):
        assert len(g["records"]) == len(e["records"]), (tag, w)
        for j, (a, b) in enumerate(zip(g["records"], e["records"])):
            assert PR.same_record(a, b), (tag, w, j, a, b)
        assert g["kept"] == e["kept"], (tag, w)
        assert (g["n_kept"], g["kept_bases"]) == (e["n_kept"], e["kept_bases"]), (tag, w)


# ---- tests/cpp/prep_host_main.cpp ------------------------------------------------

def pack(text):
    n, out = "", []
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | OPS.index(ch))
            n = ""
    return out


def host_input(windows) -> str:
    lines = [str(len(windows))]
    for w in windows:
        lines.append(f"{w['begin']} {w['end']} {len(w['reads'])}")
        for r in w["reads"]:
            words = pack(r["cigar"])
            lines.append(" ".join(str(x) for x in [r["flag"], r["mapq"], r["pos"], r["seq_len"], r["mate_same"],
                                                   len(words)] + words))
    return "\n".join(lines) + "\n"


FIELDS = ("keep", "drop_reason", "offset", "length", "new_pos", "front_to_M", "back_to_M", "begin", "end")


def parse_host_output(text):
    out, lines = [], iter(text.splitlines())
    for line in lines:
        tok = line.split()
        assert tok[0] == "W"
        n_reads, n_kept, kept_bases = int(tok[1]), int(tok[2]), int(tok[3])
        kept = [int(x) for x in tok[4:]]
        recs = [dict(zip(FIELDS, (int(x) for x in next(lines).split()))) for _ in range(n_reads)]
        out.append(dict(records=recs, kept=kept, n_kept=n_kept, kept_bases=kept_bases))
    return out


def build_host_main(tmp_path):
    exe = tmp_path / "prep_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DPREPX_HOST_ONLY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "prep_host_main.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)
