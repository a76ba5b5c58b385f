"""Seeded windows for the window caller's tests (test_gpu_call_windows.py,
test_gpu_call_dropin.py) and their expected side.

windows(n, seed): 415-base padded windows (origin = the middle 245) on a contig
with 60-base flanks, 0-3 variants each (SNPs, deletions, insertions; window 1
always has a deletion). Reads of 60-101 bases are sampled from the reference
haplotype and the variant haplotype at known offsets, so their POS and CIGAR
are known by construction. Some get soft-clipped ends (junk bases under an S) on
either strand, some hang over a window edge, and in every window with reads one
read each is removed by MAPQ, duplicate, secondary, mate contig and minimum
length. Window 2 has no reads, window 3 only reads the flag filters remove,
window 4 no variant.

expected(windows): the restatement's prepared reads (prep_restate.py on the
real strings) through hcasm.assemble, the two skip rules of call_region and
hcregion.call_regions: what hccall.call_windows must equal.
"""
from __future__ import annotations

import numpy as np

import prep_restate as PR

SEED = 20261019          # see test_gpu_call_windows.test_the_set_reaches_every_ending
N_WINDOWS = 24
WINDOW, ORIGIN_PAD, FLANK = 415, 85, 60
READS_PER_WINDOW = 150
ACGT = b"ACGT"
_ACGT = np.frombuffer(ACGT, np.uint8)

CALLED, NO_READS, NO_VARIATION = 0, 1, 2


def _bases(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def _variant_hap(rng, ext, n_variants, force_deletion):
    """The variant haplotype over the flanked reference `ext`: per haplotype base
    its position in ext (-1: inserted). Variants lie inside the origin, >= 45 apart."""
    lo, hi = FLANK + ORIGIN_PAD + 10, FLANK + WINDOW - ORIGIN_PAD - 10
    slots = list(range(lo, hi - 45, 45))
    at = sorted(rng.choice(len(slots), n_variants, replace=False)) if n_variants else []
    hap, where, p = bytearray(), [], 0
    for k, s in enumerate(at):
        v = slots[s] + int(rng.integers(0, 20))
        hap += ext[p:v]
        where += range(p, v)
        kind = "D" if (force_deletion and k == 0) else "SDI"[int(rng.integers(0, 3))]
        if kind == "S":
            alt = ACGT[(ACGT.index(ext[v]) + 1 + int(rng.integers(0, 3))) % 4]
            hap.append(alt)
            where.append(v)
            p = v + 1
        elif kind == "D":
            hap.append(ext[v])
            where.append(v)
            p = v + 1 + int(rng.integers(1, 6))
        else:
            ins = _bases(rng, int(rng.integers(1, 5)))
            hap.append(ext[v])
            where.append(v)
            hap += ins
            where += [-1] * len(ins)
            p = v + 1
    hap += ext[p:]
    where += range(p, len(ext))
    return bytes(hap), where


def _cigar(where):
    """CIGAR of a read whose bases sit at ext positions `where` (first and last aligned)."""
    out, prev = [], None
    for w in where:
        if w < 0:
            op, n = "I", 1
        else:
            if prev is not None and w > prev + 1:
                out.append(["D", w - prev - 1])
            op, n, prev = "M", 1, w
        if out and out[-1][0] == op:
            out[-1][1] += n
        else:
            out.append([op, n])
    return out


def _read(rng, hap, where, contig0, start, length, soft_clip):
    while where[start] < 0:
        start += 1
    while where[start + length - 1] < 0:
        length -= 1
    bases = bytearray(hap[start:start + length])
    cig = _cigar(where[start:start + length])
    begin = contig0 + where[start]
    flag = 0x10 if rng.random() < 0.5 else 0
    u = rng.random()
    if u < soft_clip and cig[0][0] == "M" and cig[0][1] > 14:          # soft-clipped front
        a = int(rng.integers(3, 13))
        bases[:a] = _bases(rng, a)
        cig[0][1] -= a
        cig.insert(0, ["S", a])
        begin += a
    elif u < 2 * soft_clip and cig[-1][0] == "M" and cig[-1][1] > 14:      # soft-clipped back
        a = int(rng.integers(3, 13))
        bases[len(bases) - a:] = _bases(rng, a)
        cig[-1][1] -= a
        cig.append(["S", a])
    quals = rng.integers(ord("F"), ord("J"), len(bases)).astype(np.uint8).tobytes()
    return dict(flag=flag, mapq=60, pos=begin + 1, cigar="".join(f"{n}{op}" for op, n in cig), mate_same=1,
                seq_len=len(bases), bases=bytes(bases), quals=quals)


def windows(n=N_WINDOWS, seed=SEED, reads_per_window=READS_PER_WINDOW, read_len=(60, 102), soft_clip=0.12):
    """read_len: [lo, hi) of the sampled lengths; soft_clip: the share of reads with a soft-clipped front,
    and again with a soft-clipped back (tools/call_timing.py asks for 415 reads of 101 and fewer junk ends:
    the junk under 100 soft clips alone would pass the assembler's 2000 unique k-mers)."""
    rng = np.random.default_rng(seed)
    out = []
    for w in range(n):
        padded_begin = 10_000 + 1_000 * w
        contig0 = padded_begin - FLANK                  # contig coordinate of ext[0]
        ext = _bases(rng, WINDOW + 2 * FLANK)
        n_variants = 0 if w == 4 else int(rng.integers(1, 4))
        hap, where = _variant_hap(rng, ext, n_variants, force_deletion=(w == 1))
        ref_where = list(range(len(ext)))
        sources = [(h, wh, np.maximum.accumulate(np.array(wh))) for h, wh in ((ext, ref_where), (hap, where))]
        reads = []
        for _ in range(0 if w == 2 else reads_per_window):
            length = int(rng.integers(*read_len))
            h, wh, upto = sources[int(rng.random() < 0.5)]
            # starts from 50 bases before the window to 50 before its end: both edges are overhung
            first = FLANK - 50 + int(rng.integers(0, WINDOW))
            start = min(int(np.searchsorted(upto, first)), len(h) - length)
            reads.append(_read(rng, h, wh, contig0, start, length, soft_clip))
        if reads:
            reads[5]["mapq"] = 19
            reads[17]["flag"] |= 0x400
            reads[29]["flag"] |= 0x100
            reads[41]["mate_same"] = 0
            # nine bases inside the window's end: removed for length
            reads[53] = dict(flag=0, mapq=60, pos=padded_begin + WINDOW - 9 + 1, cigar="60M", mate_same=1, seq_len=60,
                             bases=ext[FLANK + WINDOW - 9:][:60].ljust(60, b"A"), quals=b"I" * 60)
        if w == 3:
            for j, r in enumerate(reads):
                if j % 3 == 0:
                    r["mapq"] = j % 20
                elif j % 3 == 1:
                    r["flag"] |= 0x400 if j % 2 else 0x100
                else:
                    r["mate_same"] = 0
        out.append(dict(ref=ext[FLANK:FLANK + WINDOW], padded_begin=padded_begin, padded_end=padded_begin + WINDOW,
                        origin_begin=padded_begin + ORIGIN_PAD, origin_end=padded_begin + WINDOW - ORIGIN_PAD,
                        reads=reads))
    return out


def prep_window(w):
    """The window as hcprep.prep_reads and prep_restate.records take it."""
    return dict(begin=w["padded_begin"], end=w["padded_end"], reads=w["reads"])


def restated_reads(w):
    """prep_restate.prepare on the real strings: (indices of the survivors,
    [(bases, quals, begin, end)] of the survivors, the reason per read)."""
    sam = [PR.SAMRecord(r["flag"], r["pos"], r["mapq"], r["cigar"], "=" if r["mate_same"] else "chrOther",
                        r["bases"].decode("latin-1"), r["quals"].decode("latin-1")) for r in w["reads"]]
    kept, reasons = PR.prepare(sam, w["padded_begin"], w["padded_end"])
    idx = [j for j, c in enumerate(reasons) if c == PR.KEPT]
    return idx, [(s.SEQ.encode("latin-1"), s.QUAL.encode("latin-1")) + s.get_interval() for s in kept], reasons


def expected(wins):
    """The chain the parent commit already has, on the restatement's reads."""
    import hcasm
    import hcregion
    prepared = [restated_reads(w) for w in wins]
    out = [dict(status=NO_READS, asm_status=hcasm.NO_HAPLOTYPES, kmer_size=0, haps=[], reads=idx, reasons=reasons)
           for idx, _, reasons in prepared]
    to_asm = [k for k, (idx, _, _) in enumerate(prepared) if idx]
    asm = hcasm.assemble([dict(ref=wins[k]["ref"], reads=[(b, q) for b, q, _, _ in prepared[k][1]]) for k in to_asm])
    to_call = []
    for k, a in zip(to_asm, asm):
        out[k].update(status=NO_VARIATION if len(a["haps"]) <= 1 else CALLED, asm_status=a["status"],
                      kmer_size=a["kmer_size"], haps=a["haps"])
        if len(a["haps"]) > 1:
            to_call.append(k)
    regions = []
    for k in to_call:
        w, reads = wins[k], prepared[k][1]
        regions.append(dict(ref=w["ref"], padded_begin=w["padded_begin"], origin_begin=w["origin_begin"],
                            origin_end=w["origin_end"], haps=[h[0] for h in out[k]["haps"]],
                            reads=[(b, q, b"I" * len(b), b"I" * len(b), b"+" * len(b)) for b, q, _, _ in reads],
                            read_begin=np.array([r[2] for r in reads], np.int64),
                            read_end=np.array([r[3] for r in reads], np.int64)))
    sites = []
    if regions:
        got = hcregion.call_regions(regions, want_L=True, want_site_reads=True, want_cigars=True)
        for c, k in enumerate(to_call):
            out[k]["reads"] = [j for j, keep in zip(out[k]["reads"], got["keep"][c]) if keep]
            out[k]["L"] = got["L"][c]
            out[k]["alignments"] = got["alignments"][c]
        sites = [dict(s, region=to_call[s["region"]]) for s in got["sites"]]
    return dict(windows=out, sites=sites)
