"""Seeded active regions with real reads, for the region caller (include/hc_region.h).

Modelled on tests/cpp/region_pipeline.cpp::make_region: a 415-base window with a
245-base origin in its middle (HaplotypeCaller::do_work's defaults), 1-4 true
variants well apart inside the origin, the candidate haplotypes as every subset
of the variants plus, now and then, an assembly artefact (a private SNP), and a
diploid sample of two of the subsets. Reads of 100-151 bases are drawn from the
sample's two haplotypes with base errors (1 in 300), one read in 50 is junk (the
filter removes it), qualities are 20-40 and every read carries its interval on
the window. In one region of four the sample is skewed towards its first
haplotype (allelic imbalance), which gives heterozygous sites of low quality.

A region is a dict {ref, padded_begin, origin_begin, origin_end, haps: [bytes],
reads: [(bases, q, i, d, c)], read_begin, read_end}: what hcregion.call_regions
takes. Haplotypes may carry an alignment instead: {bases, begin, cigar} dicts
(with_alignments)."""
from __future__ import annotations

import numpy as np

ACGT = b"ACGT"
WINDOW, ORIGIN = 415, 245
SEED = 7   # the committed test seed (tests/test_region_capi.py asserts what it covers)


def _apply(ref: bytes, variants, mask: int) -> bytes:
    out, p = bytearray(), 0
    for k, (pos, kind, alt, ln) in enumerate(variants):
        if not mask >> k & 1:
            continue
        out += ref[p:pos]
        if kind == 0:
            out += alt
            p = pos + 1
        elif kind == 1:
            out += ref[pos:pos + 1] + alt
            p = pos + 1
        else:
            p = pos + ln
    return bytes(out + ref[p:])


def _to_ref(variants, mask: int, hpos: int) -> int:
    shift = 0
    for k, (pos, kind, alt, ln) in enumerate(variants):
        if not mask >> k & 1:
            continue
        if pos + shift >= hpos:
            break
        shift += len(alt) if kind == 1 else -ln if kind == 2 else 0
    return max(0, hpos - shift)


def region(rng, window=WINDOW, origin=ORIGIN, n_variants=(1, 4), n_reads=(40, 240), artefact=None):
    U = lambda lo, hi: int(rng.integers(lo, hi + 1))   # noqa: E731  (inclusive, as the C++ harness)
    pad = (window - origin) // 2
    ref = bytes(ACGT[U(0, 3)] for _ in range(window))
    variants = []
    nv = U(*n_variants)
    for _ in range(400):
        if len(variants) >= nv:
            break
        pos, r = U(pad + 8, pad + origin - 12), U(0, 9)
        if r < 6:
            a = ACGT[U(0, 3)]
            while a == ref[pos]:
                a = ACGT[U(0, 3)]
            v = (pos, 0, bytes([a]), 1)
        elif r < 8:
            ln = U(1, 3)
            v = (pos, 1, bytes(ACGT[U(0, 3)] for _ in range(ln)), ln)
        else:
            v = (pos, 2, b"", U(1, 3))
        if all(abs(w[0] - pos) > 8 for w in variants):
            variants.append(v)
    variants.sort()
    masks = list(range(1 << len(variants)))
    haps = [_apply(ref, variants, m) for m in masks]
    if (U(0, 2) == 0) if artefact is None else artefact:
        h = bytearray(haps[-1])
        p = U(pad, pad + origin - 1)
        h[p] = ord("C") if h[p] == ord("A") else ord("A")
        haps.append(bytes(h))
    m1, m2 = masks[U(0, len(masks) - 1)], masks[U(0, len(masks) - 1)]
    s1, s2 = _apply(ref, variants, m1), _apply(ref, variants, m2)
    p_first = 0.92 if U(0, 3) == 0 else 0.5
    reads, rb, re_ = [], [], []
    padded_begin = U(1000, 1_000_000)
    for _ in range(U(*n_reads)):
        first = rng.random() < p_first
        src = s1 if first else s2
        ln = min(U(100, 151), len(src))
        st = U(0, len(src) - ln)
        seq = bytearray(src[st:st + ln])
        qual = (33 + rng.integers(20, 41, ln)).astype(np.uint8).tobytes()
        for i in np.flatnonzero(rng.integers(0, 300, ln) == 0):
            seq[int(i)] = ACGT[U(0, 3)]
        if U(0, 49) == 0:   # a junk read the filter removes
            seq = bytearray(np.frombuffer(ACGT, np.uint8)[rng.integers(0, 4, ln)].tobytes())
        b = _to_ref(variants, m1 if first else m2, st)
        reads.append((bytes(seq), qual, b"I" * ln, b"I" * ln, b"+" * ln))
        rb.append(padded_begin + b)
        re_.append(padded_begin + min(window, b + ln))
    return dict(ref=ref, padded_begin=padded_begin, origin_begin=padded_begin + pad,
                origin_end=padded_begin + pad + origin, haps=haps, reads=reads,
                read_begin=np.array(rb, np.int64), read_end=np.array(re_, np.int64))


def regions(n=24, seed=SEED, **kw):
    rng = np.random.default_rng(seed)
    return [region(rng, **kw) for _ in range(n)]


def sized(n=512, n_reads=415, n_haps=32, seed=11):
    """The timing workload: regions of exactly n_reads reads x n_haps haplotypes
    (n_haps a power of two: every subset of log2(n_haps) variants)."""
    nv = int(n_haps).bit_length() - 1
    assert 1 << nv == n_haps
    rng = np.random.default_rng(seed)
    return [region(rng, n_variants=(nv, nv), n_reads=(n_reads, n_reads), artefact=False) for _ in range(n)]


def hap_bases(h) -> bytes:
    return h["bases"] if isinstance(h, dict) else h


def sw_batch(regs):
    """The flat batch hcsw.align_flat / oracle.SWOracle.batch take: every haplotype
    of every region against its region's window."""
    refs = b"".join(r["ref"] for r in regs)
    ref_off, ref_len, alt_off, alt_len, alts, ro = [], [], [], [], bytearray(), 0
    for r in regs:
        for h in r["haps"]:
            b = hap_bases(h)
            ref_off.append(ro)
            ref_len.append(len(r["ref"]))
            alt_off.append(len(alts))
            alt_len.append(len(b))
            alts += b
        ro += len(r["ref"])
    return dict(ref_off=np.array(ref_off, np.int64), ref_len=np.array(ref_len, np.int32),
                alt_off=np.array(alt_off, np.int64), alt_len=np.array(alt_len, np.int32),
                refs=np.frombuffer(refs, np.uint8).copy(), alts=np.frombuffer(bytes(alts), np.uint8).copy())


def with_alignments(regs, offsets, cigars):
    """The same regions with haplotypes as {bases, begin, cigar}, from the flat
    results of sw_batch's order."""
    out, k = [], 0
    for r in regs:
        haps = []
        for h in r["haps"]:
            haps.append(dict(bases=hap_bases(h), begin=int(offsets[k]), cigar=cigars[k]))
            k += 1
        out.append(dict(r, haps=haps))
    return out


def pair_batch(r):
    """One region's reads x haplotypes as the flat pair batch oracle.Oracle.pairs
    takes (read-major)."""
    haps = [hap_bases(h) for h in r["haps"]]
    hoff = np.concatenate([[0], np.cumsum([len(h) for h in haps])])[:-1]
    roff = np.concatenate([[0], np.cumsum([len(x[0]) for x in r["reads"]])])[:-1] if r["reads"] else np.zeros(0)
    nr, nh = len(r["reads"]), len(haps)
    cat = lambda k: np.frombuffer(b"".join(x[k] for x in r["reads"]) or b"\0", np.uint8).copy()   # noqa: E731
    return dict(read_off=np.repeat(roff, nh).astype(np.int64),
                R=np.repeat([len(x[0]) for x in r["reads"]], nh).astype(np.int32),
                hap_off=np.tile(hoff, nr).astype(np.int64), H=np.tile([len(h) for h in haps], nr).astype(np.int32),
                rs=cat(0), q=cat(1), ins=cat(2), dels=cat(3), gcp=cat(4),
                hap=np.frombuffer(b"".join(haps), np.uint8).copy())


def write_regions(path, regs):
    """The binary layout tests/cpp/region_call.cpp reads (int32 length-prefixed
    strings): n_regions, then per region ref, padded_begin, origin_begin,
    origin_end (int64), n_haps, the haplotypes' bases, n_reads, and per read
    bases, qualities, begin and end (int64)."""
    import struct

    def s(b):
        return struct.pack("<i", len(b)) + b

    blob = [struct.pack("<i", len(regs))]
    for r in regs:
        blob += [s(r["ref"]), struct.pack("<qqqi", r["padded_begin"], r["origin_begin"], r["origin_end"], len(r["haps"]))]
        blob += [s(hap_bases(h)) for h in r["haps"]]
        blob.append(struct.pack("<i", len(r["reads"])))
        for x, b, e in zip(r["reads"], r["read_begin"], r["read_end"]):
            blob += [s(x[0]), s(x[1]), struct.pack("<qq", int(b), int(e))]
    with open(path, "wb") as f:
        f.write(b"".join(blob))
