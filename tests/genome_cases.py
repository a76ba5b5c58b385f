"""Inputs shared by the tests of the genome caller (test_genome_restate.py,
test_genome_host.py, test_gpu_genome.py, test_gpu_genome_dropin.py), seeded and
built from sam_cases.contig() and sam_cases.flat_contig().

genome(): a table of twelve contigs, in an order that differs from the order in
which the names first appear in the file:

    chrT_alt   40 bases      chr        64 bases     chrF      9 000 bases (flat_contig)
    chrEmpty   500 bases, no reads                   chrT      the 13-window contig with its reads
    chrT2      1 base                                chrS65    65 bases
    chrOther   chrT's bases: receives the every-97th reads of sam_cases.contig()
    chrS245    245 bases     chrS246    246 bases (two windows)
    LONG_NAME  255 bytes, 130 bases                  chrU      300 bases, its reads carry a substitution

chrT2, chrT_alt and chr are prefixes and extensions of chrT and of one another.
Together the contigs have more than 16 000 positions and 76 windows, so the
position scan runs over several tiles. The read lines of all contigs are
shuffled together. Every short contig has a read at its last position and the
next contig in table order one at its position 1 (MAPQ 0 where the read
overhangs the contig: the pick takes it, the chain drops it), which catches a
window that reaches into its neighbour's positions and a read past its own
contig's end that lands in the next one. QNAMEs of 57 to 63 and of 254 bytes
put the RNAME behind the first row of 64 bytes and across row borders.

big_table(): 300 names, the twelve among 288 generated contigs without reads,
so that lookups probe past their first slot.
"""
from __future__ import annotations

import functools

import numpy as np

import call_cases as CC
import sam_cases as SC

SEED = 20261021
LONG_NAME = "chrLong_" + "n" * 247
SHORT = ("chrT_alt", "chr", "chrT2", "chrS65", "chrS245", "chrS246", LONG_NAME, "chrU")
ORDER = ("chrT_alt", "chr", "chrF", "chrEmpty", "chrT", "chrT2", "chrS65", "chrOther", "chrS245", "chrS246", LONG_NAME, "chrU")
LENGTHS = {"chrT_alt": 40, "chr": 64, "chrT2": 1, "chrEmpty": 500, "chrS65": 65, "chrS245": 245, "chrS246": 246,
           LONG_NAME: 130, "chrU": 300}
VARIANT_AT = 150     # 0-based, on chrU
QNAME_LENGTHS = (254, 57, 58, 59, 60, 61, 62, 63)
assert len(LONG_NAME) == 255 and len(ORDER) == 12


def _retarget(sam_line: str, rname: str, qname=None) -> str:
    f = sam_line.split("\t")
    f[2] = rname
    if qname is not None:
        f[0] = qname
    return "\t".join(f)


@functools.lru_cache(maxsize=None)
def genome():
    """dict(contigs = [(name, ref bytes)] in table order, sam = bytes)."""
    rng = np.random.default_rng(SEED)
    c, flat = SC.contig(), SC.flat_contig()
    refs = {"chrT": c["ref"], "chrOther": c["ref"], "chrF": flat["ref"]}
    for name, n in LENGTHS.items():
        refs[name] = CC._bases(rng, n)
    n_header = SC.HEADER.count("\n")
    lines = c["sam"].decode().split("\n")[n_header:-1]                # RNAME chrT, every 97th chrOther
    lines += [_retarget(ln, "chrF") for ln in flat["sam"].decode().split("\n")[n_header:-1]]

    # chrU's reads carry a substitution at position 151, so that the VCF has lines of a second contig
    haps = dict(refs)
    alt = bytearray(refs["chrU"])
    alt[VARIANT_AT] = CC.ACGT[(CC.ACGT.index(alt[VARIANT_AT]) + 1) % 4]
    haps["chrU"] = bytes(alt)

    def read(name, pos, length, mapq=60, tag=""):
        ref = haps[name]
        seq = (ref[pos - 1:pos - 1 + length] + b"A" * length)[:length].decode()     # an overhang reads A
        return SC.line(qname=f"{tag}{name[:8]}_{pos}", rname=name, pos=pos, mapq=mapq, seq=seq, flag=99)

    for name in SHORT:
        n = len(refs[name])
        length, step = (60, 2) if name == "chrU" else (30, 7)
        for k in range(0, n - length + 1, step):                        # whole reads inside the contig, two deep at some
            lines.append(read(name, k + 1, length))
            if k % 3 == 0:
                lines.append(read(name, k + 1, length, tag="b"))
        lines.append(read(name, n, 30, mapq=0, tag="last"))             # the contig's last position
        nxt = ORDER[(ORDER.index(name) + 1) % len(ORDER)]
        whole = len(refs[nxt]) >= 30
        lines.append(read(nxt, 1, 30, mapq=60 if whole else 0, tag="first"))
    rng.shuffle(lines)
    # long QNAMEs on reads of several contigs, the contig with the long name among them
    wanted = [LONG_NAME, "chrT", "chrF", "chr", "chrOther", "chrT_alt", "chrS246", "chrU"]
    for length, name in zip(QNAME_LENGTHS, wanted):
        k = next(i for i, ln in enumerate(lines) if ln.split("\t")[2] == name and len(ln.split("\t")[0]) < 40)
        lines[k] = _retarget(lines[k], name, qname=("Q%d_" % length).ljust(length, "q"))
    sam = (SC.HEADER + "".join(ln + "\n" for ln in lines)).encode()
    return dict(contigs=[(name, refs[name]) for name in ORDER], sam=sam)


@functools.lru_cache(maxsize=None)
def big_table():
    """300 contigs: the twelve of genome() spread among generated ones without reads."""
    rng = np.random.default_rng(SEED + 1)
    twelve = list(genome()["contigs"])
    out = []
    for k in range(288):
        if k % 24 == 5:
            out.append(twelve.pop(0))
        out.append((f"chrUn_{k * 7919 % 1000}v{k}", CC._bases(rng, 10 + k % 50)))
    assert not twelve and len(out) == 300
    return out


def first_appearance(sam: bytes):
    seen = []
    for ln in sam.decode("latin-1").split("\n"):
        f = ln.split("\t")
        if len(f) > 2 and not ln.startswith("@") and f[2] not in seen:
            seen.append(f[2])
    return seen
