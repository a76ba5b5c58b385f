"""What the GPU tests of the interval calls (test_gpu_intervals.py,
test_gpu_intervals_bam.py) share: the expected side of the stand-in rule of
include/hc_intervals.h, made from a plain call's result in Python
(intervals_restate.py decides the asked windows), and the comparison.

An interval is (contig index, begin, end), 0-based and half-open."""
from __future__ import annotations

import numpy as np

import intervals_restate as IR
from gt_restate import EMITTED

REGION, PADDING = 245, 85
NOT_ASKED, NO_READS, ASM_NO_HAPLOTYPES = 3, 1, 1
HEADER_LINES = 4
BOUNDS = ("contig", "padded_begin", "padded_end", "origin_begin", "origin_end", "ref_len")
WINDOW_FIELDS = BOUNDS + ("picked", "status", "asm_status", "kmer_size", "n_haps", "reads")
SITE_FIELDS = ("region", "status", "begin", "loc_end", "n_alleles", "alleles", "n_keep", "keep_is_null", "genotype_index",
               "a1", "a2", "genotype_quality")


def by_name(names, *intervals):
    return [(names.index(n), b, e) for n, b, e in intervals]


def whole(contigs):
    return [(c, 0, len(ref)) for c, (_, ref) in enumerate(contigs)]


def vcf_lines(plain):
    """Per emitted site of a plain call, in order: (site, its VCF line)."""
    lines = plain["vcf"].split(b"\n")[HEADER_LINES:-1]
    emitted = [s for s in plain["sites"] if s["status"] == EMITTED]
    assert len(lines) == len(emitted)
    return list(zip(emitted, lines))


def expected(plain, contigs, intervals, region=REGION, padding=PADDING):
    """The interval call that the stand-in rule makes of the plain call `plain` (with skip_unplaced)."""
    ref_lens = [len(ref) for _, ref in contigs]
    assert IR.check(intervals, ref_lens) is None
    merged = IR.merge_sorted(intervals)
    asked = IR.asked(merged, ref_lens, region, padding)
    is_asked = set(asked)
    wins = []
    for w, x in enumerate(plain["windows"]):
        if w in is_asked:
            wins.append(dict(x))
        else:
            wins.append(dict({f: x[f] for f in BOUNDS}, picked=[], status=NOT_ASKED, asm_status=ASM_NO_HAPLOTYPES, kmer_size=0,
                             n_haps=0, reads=[]))
    header = b"".join(ln + b"\n" for ln in plain["vcf"].split(b"\n")[:HEADER_LINES])
    text = [ln for s, ln in vcf_lines(plain)
            if s["region"] in is_asked and IR.inside(merged, plain["windows"][s["region"]]["contig"], s["begin"])]
    return dict(merged=merged, asked=asked, windows=wins, sites=[s for s in plain["sites"] if s["region"] in is_asked],
                vcf=header + b"".join(ln + b"\n" for ln in text), contigs=plain["contigs"])


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


def assert_sites(a, e):
    assert len(a) == len(e)
    for x, y in zip(a, e):
        for f in SITE_FIELDS:
            assert x[f] == y[f], (f, x[f], y[f])
        assert x["hap_allele"].tolist() == y["hap_allele"].tolist() and x["keep"].tolist() == y["keep"].tolist()
        assert bits(x["genotype_likelihoods"]) == bits(y["genotype_likelihoods"])


def assert_call(got, exp, what=None, contigs=True):
    """Every window field, site field and likelihood bit, the VCF bytes, the merged intervals and the asked windows;
    contigs=False where the two texts differ in records out of scope, which the contigs' record counts include."""
    assert got["merged"] == exp["merged"], what
    assert got["asked"] == exp["asked"], what
    assert len(got["windows"]) == len(exp["windows"]), what
    for k, (x, y) in enumerate(zip(got["windows"], exp["windows"])):
        for f in WINDOW_FIELDS:
            assert x[f] == y[f], (what, k, f, x[f], y[f])
    assert_sites(got["sites"], exp["sites"])
    assert got["vcf"] == exp["vcf"], what
    if contigs:
        assert got["contigs"] == exp["contigs"], what


def assert_same_records(a, e):
    for k in ("records", "line_no", "pool", "contig_of"):
        assert a["sam"][k].tobytes() == e["sam"][k].tobytes(), k


# ---- files for the indexed call: coordinate-sorted, with the index bai_writer.py makes ----------

import functools   # noqa: E402

import bam_cases as BC   # noqa: E402
import bai_writer as BW   # noqa: E402
import call_cases as CC   # noqa: E402
import genome_cases as GC   # noqa: E402
import sam_cases as SC   # noqa: E402

BIG_LEN = 300_000
CLUSTERS = tuple(8_000 + 16_384 * k for k in (0, 2, 4, 7, 9, 12, 15, 17))   # each in a 16 KiB stretch of its own
STRADDLERS = (16_384, 131_072, 262_144)


def sorted_text(sam, order):
    """The text's alignment lines sorted by (the name's place in `order`, POS), file order kept within a position."""
    lines = sam.decode("latin-1").split("\n")
    head = [ln for ln in lines if ln.startswith("@")]
    body = [ln for ln in lines if ln and not ln.startswith("@")]
    body.sort(key=lambda ln: (order.index(ln.split("\t")[2]), int(ln.split("\t")[3])))
    return "".join(ln + "\n" for ln in head + body).encode("latin-1")


@functools.lru_cache(maxsize=None)
def sorted_genome(member_size):
    """The twelve contigs of genome_cases.py sorted by (header order, POS); the BAM header lists the references in the
    reverse of the table's order. dict(contigs, refs, sam, bam, bai, ref_of: contig index -> refID)."""
    g = GC.genome()
    refs = [(n, len(r)) for n, r in reversed(g["contigs"])]
    sam = sorted_text(g["sam"], [n for n, _ in refs])
    bam = BC.to_bam(sam, refs, member_size=member_size)
    n = len(refs)
    return dict(contigs=g["contigs"], refs=refs, sam=sam, bam=bam, bai=BW.build(bam), ref_of=[n - 1 - c for c in range(n)])


@functools.lru_cache(maxsize=None)
def big_contig():
    """chrBig, 300 000 bases: eight clusters of 40 reads of 60 bases, each cluster in its own 16 KiB stretch and with a
    substitution in its middle, and one read astride each of 16 384, 131 072 and 262 144. Members of 1 024 bytes."""
    rng = np.random.default_rng(GC.SEED + 26)
    ref = CC._bases(rng, BIG_LEN)
    alt = bytearray(ref)
    for c in CLUSTERS:
        alt[c + 60] = CC.ACGT[(CC.ACGT.index(alt[c + 60]) + 1) % 4]
    alt = bytes(alt)
    reads = [(c + 3 * k, f"c{c}_{k}") for c in CLUSTERS for k in range(40)] + [(s - 30, f"s{s}") for s in STRADDLERS]
    reads.sort()
    header = f"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrBig\tLN:{BIG_LEN}\n"
    sam = (header + "".join(SC.line(qname=q, rname="chrBig", pos=p + 1, seq=alt[p:p + 60].decode(), flag=99) + "\n"
                            for p, q in reads)).encode()
    bam = BC.to_bam(sam, [("chrBig", BIG_LEN)], member_size=1024)
    return dict(contigs=[("chrBig", ref)], refs=[("chrBig", BIG_LEN)], sam=sam, bam=bam, bai=BW.build(bam), ref_of=[0])


BIG_SETS = {
    "one_cluster": [(0, CLUSTERS[3] + 55, CLUSTERS[3] + 65)],
    "two_clusters": [(0, CLUSTERS[1] + 60, CLUSTERS[1] + 61), (0, CLUSTERS[6], CLUSTERS[6] + 200)],
    "straddlers": [(0, s - 1, s + 1) for s in STRADDLERS],
}


def restated_members(f, intervals, region=REGION, padding=PADDING):
    """(the members the specification's query reads, the header's members, all members) of file dict f, as offsets."""
    mem, stream, _, recs = BW.layout(f["bam"])
    first_record = recs[0][0] if recs else len(stream)
    header = [coff for coff, first, isize in mem if first < first_record and isize]
    chosen = IR.chosen_members(f["bai"], intervals, [len(r) for _, r in f["contigs"]], f["ref_of"], region, padding,
                               [coff for coff, _, _ in mem])
    return chosen, header, [coff for coff, _, _ in mem]
