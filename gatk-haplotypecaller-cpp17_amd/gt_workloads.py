"""Seeded synthetic genotyping sites.

A site is what Genetyper::assign_genotype_likelihoods hands to the likelihood
arithmetic for one variant start (reference genotyper/genotyper.hpp:369-399):
the region's read-major log10 likelihood matrix L (n_reads x n_haps, after
IntelPairHMM::compute_likelihoods' normalisation: every value within 4.5 of its
read's best), the reads overlapping the allele window (get_read_indices_to_keep,
:234-243), the haplotype -> allele map (get_haplotype_mapper, :224-232) and the
allele count (2..MAX_ALLELE_COUNT = 7). Several sites share a region's L.
"""
from __future__ import annotations

import numpy as np

MAX_ALLELES = 7


def region_matrix(rng, n_reads, n_haps, with_inf=False):
    """log10 likelihoods shaped like normalised PairHMM output."""
    L = -rng.gamma(2.0, 8.0, size=(n_reads, n_haps)) - rng.uniform(0, 3, size=(n_reads, 1))
    best = L.max(axis=1, keepdims=True)
    L = np.maximum(L, best - 4.5)   # intel_pairhmm.hpp:29-33
    # reads that support one hap exactly tie with it
    if n_haps > 1:
        ties = rng.random(n_reads) < 0.2
        L[ties, 1] = L[ties, 0]
    if with_inf:
        L[rng.random(L.shape) < 0.01] = -np.inf
    return np.ascontiguousarray(L, np.float64)


def sites(n_regions=16, sites_per_region=8, reads=(50, 415), haps=(2, 32), seed=61, with_inf=False):
    """Returns (matrices, sites): matrices = list of L arrays; sites = list of
    dicts {m (matrix index), keep int32[], hap_allele int32[], n_alleles}."""
    rng = np.random.default_rng(seed)
    mats, out = [], []
    for _ in range(n_regions):
        nr = int(rng.integers(reads[0], reads[1] + 1))
        nh = int(rng.integers(haps[0], haps[1] + 1))
        mats.append(region_matrix(rng, nr, nh, with_inf))
        for _ in range(sites_per_region):
            A = int(rng.integers(2, min(MAX_ALLELES, nh + 1) + 1)) if nh >= 2 else 2
            keep = np.sort(rng.choice(nr, size=int(rng.integers(1, nr + 1)), replace=False)).astype(np.int32)
            amap = rng.integers(0, A, size=nh).astype(np.int32)
            amap[0] = 0
            out.append(dict(m=len(mats) - 1, keep=keep, hap_allele=amap, n_alleles=A))
    return mats, out


def n_genotypes(a: int) -> int:
    return a * (a + 1) // 2


# ---- whole regions for hc_gt_call_regions (reference window, aligned haplotypes, reads, L) ----

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _edit_pool(rng, ref, lo, hi, n_edits):
    """Candidate edits of a region, shared by its haplotypes: (pos, order, kind,
    payload). 'S' replaces ref[pos]; 'I' inserts after ref[pos]; 'D' deletes
    ref[pos+1 : pos+1+len]. Some positions carry several SNP alts, a SNP under a
    deletion of another edit, a SNP + insertion + deletion on one anchor, or an
    insertion right behind a deletion: the cases the bookkeeping has to order."""
    pool = []
    for _ in range(n_edits):
        pos = int(rng.integers(lo, hi))
        k = rng.random()
        other = [b for b in ACGT if b != ref[pos]]
        if k < 0.45:
            pool.append((pos, 0, "S", int(other[int(rng.integers(0, 3))])))
            if rng.random() < 0.3:
                pool.append((pos, 0, "S", int(other[int(rng.integers(0, 3))])))
        elif k < 0.7:
            pool.append((pos, 1, "I", ACGT[rng.integers(0, 4, int(rng.integers(1, 7)))].tobytes()))
            if rng.random() < 0.3:
                pool.append((pos, 0, "S", int(other[0])))
        else:
            ln = int(rng.integers(1, 13))
            pool.append((pos, 2, "D", ln))
            if rng.random() < 0.5:   # a SNP of other haplotypes under the deletion
                q = pos + 1 + int(rng.integers(0, ln))
                pool.append((q, 0, "S", int([b for b in ACGT if b != ref[q]][0])))
            if rng.random() < 0.3:   # ...D I...
                pool.append((pos + ln, 1, "I", ACGT[rng.integers(0, 4, int(rng.integers(1, 4)))].tobytes()))
            if rng.random() < 0.2:   # ...I D... on one anchor
                pool.append((pos, 1, "I", ACGT[rng.integers(0, 4, 2)].tobytes()))
    return sorted(set(pool), key=lambda e: (e[0], e[1], str(e[3])))


def apply_edits(ref, edits, begin=0, end=None, lead=b"", trail=b""):
    """Haplotype bases, CIGAR text and the edits that took effect, from an edit
    script applied to ref[begin:end] (edits sorted by (pos, S < I < D); one that
    starts inside what an earlier one consumed is dropped). lead / trail are
    unaligned bases, soft-clipped."""
    end = len(ref) if end is None else end
    ops, out, used = [], bytearray(lead), []
    if lead:
        ops.append([len(lead), "S"])

    def emit(n, op):
        if n > 0:
            if ops and ops[-1][1] == op:
                ops[-1][0] += n
            else:
                ops.append([n, op])

    cur = begin
    for k, (pos, _, kind, pay) in enumerate(edits):
        if kind == "S":
            if pos < cur or pos >= end:
                continue
            out += ref[cur:pos] + bytes([pay])
            emit(pos - cur + 1, "M")
            cur = pos + 1
        elif kind == "I":
            if pos + 1 < cur or pos + 1 > end:
                continue
            out += ref[cur:pos + 1] + pay
            emit(pos + 1 - cur, "M")
            emit(len(pay), "I")
            cur = pos + 1
        else:
            if pos + 1 < cur or pos + 1 + pay > end:
                continue
            out += ref[cur:pos + 1]
            emit(pos + 1 - cur, "M")
            emit(pay, "D")
            cur = pos + 1 + pay
        used.append(k)
    out += ref[cur:end]
    emit(end - cur, "M")
    out += trail
    emit(len(trail), "S")
    return bytes(out), "".join(f"{n}{op}" for n, op in ops), used


def regions(n_regions=24, window=415, origin=245, haps=(8, 32), reads=(50, 120), seed=71):
    """Seeded regions in the layout hcgt.call_regions takes: dicts {ref,
    padded_begin, origin_begin, origin_end, haps: [{bases, begin, cigar}],
    read_begin, read_end, L}. Haplotype 0 is the reference path; the others apply
    a random subset of the region's edit pool, some with trimmed ends (a non-zero
    begin) or soft-clipped ends. Each read follows one of the two haplotypes of
    the region's genotype: L falls with the number of edits inside the read by
    which a haplotype differs from it, strongly in most regions and weakly in
    some (low qualities)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_regions):
        ref = ACGT[rng.integers(0, 4, window)].tobytes()
        padded_begin = int(rng.integers(1000, 1_000_000))
        origin_begin = padded_begin + (window - origin) // 2
        margin = min(40, max(window // 4, 1))
        pool = _edit_pool(rng, ref, margin, max(window - margin - 14, margin + 1), int(rng.integers(4, 10)))
        nh = int(rng.integers(haps[0], haps[1] + 1))
        hl, sets = [], []
        for h in range(nh):
            pick = [e for e in pool if h and rng.random() < 0.3]
            b = int(rng.integers(0, 20)) if h and rng.random() < 0.3 and window > 100 else 0
            e = window - (int(rng.integers(0, 20)) if h and rng.random() < 0.3 and window > 100 else 0)
            lead = ACGT[rng.integers(0, 4, int(rng.integers(1, 6)))].tobytes() if h and rng.random() < 0.15 else b""
            trail = ACGT[rng.integers(0, 4, int(rng.integers(1, 6)))].tobytes() if h and rng.random() < 0.15 else b""
            bases, cigar, used = apply_edits(ref, pick, b, e, lead, trail)
            hl.append(dict(bases=bases, begin=b, cigar=cigar))
            sets.append({pick[k] for k in used})
        nr = int(rng.integers(reads[0], reads[1] + 1))
        rb = padded_begin + rng.integers(-60, window - 40, nr)
        re_ = rb + rng.integers(70, 151, nr)
        t = rng.random()
        h1 = 0 if t < 0.75 else int(rng.integers(0, nh))
        h2 = 0 if t < 0.25 else int(rng.integers(0, nh))
        scale = 2.0 if rng.random() < 0.7 else 0.04
        L = np.zeros((nr, nh))
        for r in range(nr):
            truth = sets[h1 if rng.random() < 0.5 else h2]
            for h in range(nh):
                d = sum(1 for e in truth ^ sets[h] if rb[r] <= padded_begin + e[0] < re_[r])
                L[r, h] = -min(4.5, scale * d + rng.uniform(0, 0.02))
        out.append(dict(ref=ref, padded_begin=padded_begin, origin_begin=origin_begin,
                        origin_end=origin_begin + origin, haps=hl, read_begin=rb.astype(np.int64),
                        read_end=re_.astype(np.int64), L=np.ascontiguousarray(L, np.float64)))
    return out


def write_regions(path, regs):
    """The binary layout tests/cpp/gt_dropin.cpp reads (int32 length-prefixed strings)."""
    import struct

    def s(b):
        return struct.pack("<i", len(b)) + b

    blob = [struct.pack("<i", len(regs))]
    for r in regs:
        blob += [s(r["ref"]), struct.pack("<qqqi", r["padded_begin"], r["origin_begin"], r["origin_end"], len(r["haps"]))]
        for h in r["haps"]:
            blob += [s(h["bases"]), struct.pack("<i", h["begin"]), s(h["cigar"].encode())]
        blob += [struct.pack("<i", len(r["read_begin"])), np.ascontiguousarray(r["read_begin"], np.int64).tobytes(),
                 np.ascontiguousarray(r["read_end"], np.int64).tobytes(),
                 np.ascontiguousarray(r["L"], np.float64).tobytes()]
    with open(path, "wb") as f:
        f.write(b"".join(blob))
