"""Seeded assembler scenarios (a..m of the asm tests) and random regions.

A region is {"ref": bytes, "reads": [(bases, quals), ...]}. Every scenario
comes with a check(res) that asserts, on the restatement's result, the property
the scenario exists for, so a scenario cannot silently stop exercising its path.
"""
from __future__ import annotations

import random

import asm_restate as AR

ACGT = b"ACGT"


def rand_seq(rng, n):
    return bytes(rng.choice(ACGT) for _ in range(n))


def snp(seq, pos):
    alt = ACGT[(ACGT.index(seq[pos]) + 1) % 4]
    return seq[:pos] + bytes([alt]) + seq[pos + 1:]


def sample_reads(rng, hap, n, length, err=0.0, qual=ord("I")):
    out = []
    length = min(length, len(hap))
    for _ in range(n):
        s = rng.randrange(0, len(hap) - length + 1)
        b = bytearray(hap[s:s + length])
        for i in range(length):
            if err and rng.random() < err:
                b[i] = ACGT[(ACGT.index(b[i]) + 1 + rng.randrange(3)) % 4]
        out.append((bytes(b), bytes([qual]) * length))
    return out


def region(ref, reads):
    return {"ref": ref, "reads": list(reads)}


def _accepted_at(res, k):
    assert res["status"] == AR.OK and res["kmer_size"] == k, (res["status"], res["kmer_size"], res["attempts"])


def scenarios():
    """[(name, region, check)] in the order of the issue's table."""
    out = []

    def add(name, reg, check):
        out.append((name, reg, check))

    # a: one haplotype
    rng = random.Random(101)
    ref = rand_seq(rng, 200)

    def chk_a(res):
        _accepted_at(res, 25)
        assert len(res["haps"]) == 1 and res["haps"][0][0] == res["g"].ref
    add("a", region(ref, sample_reads(rng, ref, 30, 80)), chk_a)

    # b: SNP
    rng = random.Random(102)
    ref_b = rand_seq(rng, 200)
    alt_b = snp(ref_b, 100)
    reads_b = sample_reads(rng, ref_b, 20, 80) + sample_reads(rng, alt_b, 20, 80)

    def chk_b(res):
        _accepted_at(res, 25)
        assert len(res["haps"]) == 2 and res["haps"][0][1] != res["haps"][1][1]
        assert {h[0] for h in res["haps"]} == {ref_b, alt_b}
    add("b", region(ref_b, reads_b), chk_b)

    # c: 7-base deletion
    rng = random.Random(103)
    ref_c = rand_seq(rng, 220)
    alt_c = ref_c[:110] + ref_c[117:]

    def chk_c(res):
        _accepted_at(res, 25)
        assert {h[0] for h in res["haps"]} == {ref_c, alt_c}
    add("c", region(ref_c, sample_reads(rng, ref_c, 20, 80) + sample_reads(rng, alt_c, 20, 80)), chk_c)

    # d: (b) with 1 % read errors
    rng = random.Random(104)
    reads_d = sample_reads(rng, ref_b, 20, 80, err=0.01) + sample_reads(rng, alt_b, 20, 80, err=0.01)

    def chk_d(res):
        _accepted_at(res, 25)
        assert {h[0] for h in res["haps"]} == {ref_b, alt_b}
        g = res["g"]
        assert len(g.edges) > len(res["graph"])            # error edges exist and are not on path
        assert any(not g.edge_filter(e) for e in g.edges)  # some are filtered
    add("d", region(ref_b, reads_d), chk_d)

    # e: duplicate k-mers
    rng = random.Random(105)
    ref_e = rand_seq(rng, 60) + b"ACGTTGCA" * 6 + rand_seq(rng, 60)

    def chk_e(res):
        _accepted_at(res, 25)
        g = res["g"]
        assert g.dup_kmers and len(g.kmer) > g.unique_kmers_count()
    add("e", region(ref_e, sample_reads(rng, ref_e, 40, 70)), chk_e)

    # f: tandem duplication seen only at its junction
    rng = random.Random(106)
    P, U, Q = rand_seq(rng, 80), rand_seq(rng, 30), rand_seq(rng, 80)
    uu = U + U
    reads_f = [(uu[o:o + 44], b"I" * 44) for _ in range(3) for o in range(0, 17)]

    def chk_f(res):
        assert res["attempts"][:2] == [AR.CYCLE, AR.ACCEPTED], res["attempts"]
        _accepted_at(res, 35)
    add("f", region(P + U + Q, reads_f), chk_f)

    # g: too many k-mers
    rng = random.Random(107)
    ref_g = rand_seq(rng, 200)
    reads_g = [(rand_seq(rng, 101), b"I" * 101) for _ in range(30)]

    def chk_g(res):
        assert res["attempts"][:3] == [AR.TOO_MANY_KMERS, AR.TOO_MANY_KMERS, AR.ACCEPTED], res["attempts"]
        _accepted_at(res, 45)
    add("g", region(ref_g, reads_g), chk_g)

    # h: window shorter than every k
    rng = random.Random(108)

    def chk_h(res):
        assert res["attempts"] == [AR.SHORT_REF] * 9 and res["status"] == AR.NO_HAPLOTYPES and not res["haps"]
    add("h", region(rand_seq(rng, 20), sample_reads(rng, rand_seq(rng, 120), 5, 80)), chk_h)

    # i: eight independent SNPs, 256 paths
    rng = random.Random(110)   # a seed at which every alternative branch is seen at least twice
    ref_i = rand_seq(rng, 340)
    alt_i = ref_i
    for s in range(8):
        alt_i = snp(alt_i, 30 + 40 * s)

    def chk_i(res):
        _accepted_at(res, 25)
        assert res["n_paths"] == 256 and len(res["haps"]) == 128
    add("i", region(ref_i, sample_reads(rng, ref_i, 150, 36) + sample_reads(rng, alt_i, 150, 36)), chk_i)

    # j: unusable bases split the reads
    rng = random.Random(110)
    ref_j = rand_seq(rng, 200)
    alt_j = snp(ref_j, 90)
    reads_j = []
    for n, (b, q) in enumerate(sample_reads(rng, ref_j, 15, 80) + sample_reads(rng, alt_j, 15, 80)):
        b, q = bytearray(b), bytearray(q)
        at = 10 + (n * 7) % 60   # pieces on both sides of k = 25
        if n % 3 == 0:
            q[at] = ord("#")
        elif n % 3 == 1:
            b[at] = ord("N")
        else:
            q[at] = 0x80 + (n % 100)   # negative as a signed char
        if n % 5 == 0:
            q[79] = ord("*")           # quality 9, just under the threshold
        if n % 5 == 1:
            q[0] = ord("+")            # quality 10, just at it
        reads_j.append((bytes(b), bytes(q)))

    def chk_j(res):
        _accepted_at(res, 25)
        g = res["g"]
        assert len(g.read_segs) > len(reads_j) * 1.2        # reads were split
        assert len(g.read_segs) < len(reads_j) * 2          # and short pieces dropped
        assert all(len(s) >= 25 for s in g.read_segs)
    add("j", region(ref_j, reads_j), chk_j)

    # k: no reads
    rng = random.Random(111)
    ref_k = rand_seq(rng, 150)

    def chk_k(res):
        _accepted_at(res, 25)
        assert res["haps"] == [(ref_k, 0.0)]
    add("k", region(ref_k, []), chk_k)

    # l: a read that starts on a vertex of in-degree 2 (the first k-mer behind the SNP's bubble)
    rng = random.Random(112)
    ref_l = rand_seq(rng, 200)
    alt_l = snp(ref_l, 100)
    reads_l = sample_reads(rng, ref_l, 20, 80) + sample_reads(rng, alt_l, 20, 80)
    reads_l += [(ref_l[101:171], b"I" * 70)] * 2

    def chk_l(res):
        _accepted_at(res, 25)
        g = res["g"]
        assert len(g.in_edges[g.unique_kmers[ref_l[101:126]]]) == 2
        assert len(res["haps"]) == 2
    add("l", region(ref_l, reads_l), chk_l)

    # m: a read that starts mid-chain: the backward walk runs its k-1 steps
    rng = random.Random(113)
    ref_m = rand_seq(rng, 200)
    reads_m = sample_reads(rng, ref_m, 10, 80) + [(ref_m[60:140], b"I" * 80)]

    def chk_m(res):
        _accepted_at(res, 25)
        g = res["g"]
        v = g.unique_kmers[ref_m[60:85]]
        for _ in range(24):
            assert len(g.in_edges[v]) == 1
            v = g.in_edges[v][0].u
    add("m", region(ref_m, reads_m), chk_m)
    return out


def random_region(seed, window=(120, 380), reads=(40, 300), read_len=101, err=0.005):
    """Window, 0-3 variants (SNP, insertion, deletion) on one alternative
    haplotype, reads from both with sequencing errors and a few low qualities."""
    rng = random.Random(seed)
    ref = rand_seq(rng, rng.randint(*window))
    alt = ref
    nvar = rng.randint(0, 3)
    for pos in sorted((rng.randrange(30, len(ref) - 30) for _ in range(nvar)), reverse=True):
        kind = rng.randrange(3)
        if kind == 0:
            alt = snp(alt, pos)
        elif kind == 1:
            alt = alt[:pos] + rand_seq(rng, rng.randint(1, 8)) + alt[pos:]
        else:
            alt = alt[:pos] + alt[pos + rng.randint(1, 8):]
    n = rng.randint(*reads)
    out = []
    for j in range(n):
        hap = alt if (nvar and j % 2) else ref
        (b, q), = sample_reads(rng, hap, 1, rng.randint(40, read_len), err=err)
        if rng.random() < 0.1:
            q = bytearray(q)
            q[rng.randrange(len(q))] = ord("#")
            q = bytes(q)
        out.append((b, q))
    return region(ref, out)


RANDOM_SEEDS = list(range(7000, 7064))
