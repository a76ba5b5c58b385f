"""Inputs of the reference pins (test_ref_pins.py, test_gpu_ref_pins.py,
golden/make_chain_golden.py): per stage the fixed cases the committed fixture
holds, and seeded random cases for the live comparison against
oracle/_ref/libref_chain.so.

A stage's cases are a list of (name, input) pairs; an input is plain data
(str / int / list / dict, doubles as numpy arrays) that encode() turns into the
fixture's JSON, so neither test file needs this module's generators to agree
with the generator's run: they read the inputs back from the fixture.

    parse        a SAM line (str, latin-1)
    prepare      {begin, end, reads: [{flag, mapq, pos, cigar, mate_same, seq, qual}]}
    align        {ref, alt, params}
    likelihoods  {reads: [(seq, qual)], haps: [str]}
    normalize    {read_len: [int], L: float64[n_reads, n_haps]}
    genotype     a region of hcgt.call_regions: {ref, padded_begin, origin_begin,
                 origin_end, haps: [{bases, begin, cigar}], read_begin, read_end, L}
    chain        {ref, padded_begin, origin_begin, origin_end, haps: [str], reads: as prepare}
"""
from __future__ import annotations

import numpy as np

import gt_workloads as G
import prep_cases as PC
import region_workloads as RW
import sam_cases as SC
import sw_workloads as SWW

ACGT = b"ACGT"
NEW_SW_PARAMETERS = (200, -150, -260, -11)


def _bases(rng, n) -> str:
    return bytes(ACGT[int(k)] for k in rng.integers(0, 4, n)).decode()


def _other(base: str, k: int = 1) -> str:
    return "ACGT"[("ACGT".index(base) + k) % 4]


# ---- parse ---------------------------------------------------------------------------

def parse_cases():
    L = SC.line
    out = [(f"grid{k:04d}", x) for k, x in enumerate(SC.grid_lines())]
    out += [("err_" + name, bad) for name, bad, _ in SC.error_lines()]
    out += [
        ("tlen_minus_zero", L(tlen="-0")),
        ("tlen_minus_zeros", L(tlen="-000")),
        ("tlen_leading_zeros", L(tlen="-0000000000000000000017")),
        ("flag_leading_zeros_long", L(flag="0" * 40 + "16")),
        ("pos_leading_zeros_long", L(pos="0" * 40 + "7")),
        ("mapq_zero_zero", L(mapq="00")),
        ("pnext_max", L(pnext=4294967295)),
        ("pnext_overflow", L(pnext=4294967296)),
        ("pnext_plus", L(pnext="+3")),
        ("flag_plus", L(flag="+4")),
        ("mapq_plus", L(mapq="+4")),
        ("mapq_overflow", L(mapq=65536)),
        ("tlen_min", L(tlen=-2147483648)),
        ("stars_all", L(cigar="*", rnext="*", seq="*", qual="*")),
        ("cigar_zero_length", L(cigar="0M4M")),
        ("tags_many", L(tags=("NM:i:1", "MD:Z:4", "AS:i:4", "XS:i:0"))),
        ("trailing_separators", L() + " \t\v\f\r"),
        ("eleven_fields_then_newline_free_text", L(tags=("x y z",))),
    ]
    out += [(f"sep_{ord(c):02x}", L(sep=c)) for c in " \t\v\f\r"]
    out += [(f"sep_pair_{ord(a):02x}_{ord(b):02x}", L(sep=a + b)) for a in " \t" for b in "\v\f\r"]
    return out


def parse_random(seed, n=300):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        seq = _bases(rng, int(rng.integers(1, 120)))
        ops = []
        for _ in range(int(rng.integers(1, 6))):
            ops.append(f"{int(rng.integers(0, 300))}{'MIDNSHP=X'[int(rng.integers(0, 9))]}")
        num = lambda lo, hi: str(int(rng.integers(lo, hi)))   # noqa: E731
        pad = lambda s: "0" * int(rng.integers(0, 3)) + s   # noqa: E731
        sep = [" ", "\t", " \t", "\v", "\f\r"][int(rng.integers(0, 5))]
        out.append((f"r{k}", SC.line(qname=f"q{k}", flag=pad(num(0, 65536)), pos=pad(num(0, 2 ** 32)),
                                     mapq=pad(num(0, 65536)), cigar="".join(ops) if rng.random() < 0.9 else "*",
                                     rnext=["=", "*", "chr2"][int(rng.integers(0, 3))], pnext=num(0, 2 ** 32),
                                     tlen=("-" if rng.random() < 0.5 else "") + pad(num(0, 2 ** 31)), seq=seq,
                                     qual="I" * len(seq), sep=sep)))
    return out


# ---- prepare -------------------------------------------------------------------------

def seq_of(n: int) -> str:
    """n <= 200 distinct one-byte symbols without whitespace: a surviving slice names its own offset."""
    assert n <= 200
    return bytes(33 + k for k in range(n)).decode("latin-1")


def qual_of(n: int) -> str:
    return bytes(255 - k for k in range(n)).decode("latin-1")


def _with_text(r):
    return dict(flag=r["flag"], mapq=r["mapq"], pos=r["pos"], cigar=r["cigar"], mate_same=r["mate_same"],
                seq=seq_of(r["seq_len"]), qual=qual_of(r["seq_len"]))


def _win(w):
    return dict(begin=w["begin"], end=w["end"], reads=[_with_text(r) for r in w["reads"]])


def prepare_cases():
    out = [(f"grid{k}", _win(w)) for k, w in enumerate(PC.grid())]
    out += [(f"compaction{k}", _win(w)) for k, w in enumerate(PC.compaction())]
    R = PC.read
    edges = []
    for rev in (False, True):
        # a 30M read ending one before, at and one past the window's begin; beginning there; the same at its end
        for b in (969, 970, 971, 999, 1000, 1001, 1369, 1370, 1371, 1399, 1400, 1401):
            edges.append(R("30M", b, rev, seq_len=30))
        # 9 and 10 bases left on either side
        for b in (979, 980, 1390, 1391):
            edges.append(R("30M", b, rev, seq_len=30))
        edges += [R("30S", 1100, rev, seq_len=30),                 # one element that is front() and back()
                  R("1S", 1100, rev, seq_len=1), R("10S", 1005, rev, seq_len=10),
                  R("10M100D10M", 1340, rev, seq_len=20),          # the end clip is larger than the read
                  R("10M500D10M", 950, rev, seq_len=20),           # both clips, the first takes every base
                  R("12S20M12S", 1000, rev, seq_len=44), R("12S20M12S", 1388, rev, seq_len=44),
                  R("5H10S20M10S5H", 1100, rev, seq_len=40), R("200M", 1100, rev, seq_len=200)]
    out.append(("edges", _win(dict(begin=1000, end=1400, reads=edges))))
    low = []
    for fl in (1, 2, 7):
        for b in (0, 1, fl - 1, fl, fl + 1):
            if b >= 0:
                low += [R(f"{fl}S{30 - fl}M", b, rev, seq_len=30) for rev in (False, True)]
    out.append(("contig_start", _win(dict(begin=0, end=300, reads=low))))
    out.append(("contig_start_clipped", _win(dict(begin=3, end=25, reads=low))))
    # what include/hc_prep.h refuses, one read per window, each also behind a flag filter (where nobody looks at it)
    ok = R("40M", 1100)
    for name, bad in (("pos_zero", dict(R("40M", 1100), pos=0)),
                      ("cigar_shorter_than_seq", R("39M", 1100)),
                      ("cigar_longer_than_seq", R("30M20S", 1100)),
                      ("front_clip_past_the_read", R("50S", 1100, True))):
        out.append((f"refused_{name}", _win(dict(begin=1000, end=1400, reads=[ok, bad, ok]))))
        out.append((f"filtered_{name}", _win(dict(begin=1000, end=1400, reads=[ok, dict(bad, mapq=3), ok]))))
    return out


def prepare_random(seed, n=200):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        begin = int(rng.integers(0, 3)) * 500
        end = begin + int(rng.integers(20, 420))
        reads = []
        for _ in range(int(rng.integers(0, 12))):
            ops, n_read = [], 0
            if rng.random() < 0.3:
                ops.append(f"{int(rng.integers(1, 6))}H")
            shape = [("S", 0.4), ("M", 1.0), ("I", 0.3), ("M", 0.3), ("D", 0.3), ("N", 0.1), ("=", 0.2), ("X", 0.2),
                     ("M", 0.5), ("S", 0.4)]
            for op, p in shape:
                if rng.random() < p:
                    ln = int(rng.integers(1, 25))
                    ops.append(f"{ln}{op}")
                    n_read += ln if op in "MIS=X" else 0
            if n_read == 0:
                ops.append("7M")
                n_read = 7
            pos = max(1, begin + int(rng.integers(-60, end - begin + 30)))
            reads.append(dict(flag=int(rng.choice([0, 0x10, 0x400, 0x100, 0x10 | 0x1])), mapq=int(rng.choice([60, 20, 19, 0])),
                              pos=pos, cigar="".join(ops), mate_same=int(rng.random() < 0.9), seq=seq_of(n_read),
                              qual=qual_of(n_read)))
        out.append((f"r{k}", dict(begin=begin, end=end, reads=reads)))
    return out


# ---- align ---------------------------------------------------------------------------

def _pair(ref, alt, params=NEW_SW_PARAMETERS):
    return dict(ref=ref, alt=alt, params=list(params))


def align_cases(sw_golden_sets=None):
    rng = np.random.default_rng(301)
    out = []
    r = _bases(rng, 80)
    mism = lambda k: "".join(_other(c) if i in (7, 40, 79)[:k] else c for i, c in enumerate(r))   # noqa: E731
    out += [("equal_0_mismatches", _pair(r, r)), ("equal_2_mismatches", _pair(r, mism(2))),
            ("equal_3_mismatches", _pair(r, mism(3))), ("equal_1_mismatch", _pair(r, mism(1))),
            ("one_base_equal", _pair("A", "A")), ("one_base_differs", _pair("A", "C")),
            ("two_bases_differ", _pair("AC", "CA")), ("three_bases_differ", _pair("ACG", "CAT")),
            ("shorter", _pair(r, r[5:70])), ("longer", _pair(r[5:70], r)),
            ("leading_trailing_junk", _pair(r, _bases(rng, 6) + r[10:70] + _bases(rng, 6))),
            ("leading_extra", _pair(r, "GGGGG" + r)), ("trailing_extra", _pair(r, r + "GGGGG")),
            ("leading_missing", _pair(r, r[4:])), ("trailing_missing", _pair(r, r[:-4])),
            ("insertion_near_start", _pair(r, r[:3] + "TTTT" + r[3:])),
            ("deletion_near_start", _pair(r, r[:3] + r[9:])),
            ("insertion_near_end", _pair(r, r[:-3] + "TTTT" + r[-3:])),
            ("deletion_near_end", _pair(r, r[:-9] + r[-3:])),
            ("unrelated", _pair(r, _bases(rng, 50)))]
    for p in SWW.PARAM_SETS[1:]:
        out.append((f"params_{p[0]}", _pair(r, r[:30] + "ACG" + r[30:60] + r[64:], p)))
    for k, (a, b) in enumerate(SWW.edge_pairs()):
        if len(a) <= 130 and len(b) <= 130 and not set(a + b) & set(b" \t\n\v\f\r\0"):
            out.append((f"edge{k:03d}", _pair(a.decode("latin-1"), b.decode("latin-1"))))
    batch = SWW.regions(3, 6, (150, 260), seed=302)
    for k in range(len(batch["ref_len"])):
        a, b = SWW.pair(batch, k)
        out.append((f"region{k:02d}", _pair(a.decode(), b.decode())))
    return out


def align_random(seed, n=200):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        w = SWW._window(rng, int(rng.integers(1, 160)))
        u = rng.random()
        if u < 0.3:   # equal lengths, 0 .. 4 mismatches: either side of the shortcut
            a = w.copy()
            pos = rng.choice(len(w), size=min(int(rng.integers(0, 5)), len(w)), replace=False)
            a[pos] = SWW.ACGT[(np.searchsorted(SWW.ACGT, a[pos]) + 1) % 4]
        else:
            a = SWW._mutate(rng, w, 0.03, 0.02, 0.5)
        out.append((f"r{k}", _pair(w.tobytes().decode(), a.tobytes().decode(),
                                   SWW.PARAM_SETS[int(rng.integers(0, 4))] if u > 0.8 else NEW_SW_PARAMETERS)))
    return out


# ---- likelihoods ---------------------------------------------------------------------

def _read_from(rng, hap: str, n: int, errors: int, q_lo=20, q_hi=41, start=None):
    start = int(rng.integers(0, len(hap) - n + 1)) if start is None else start
    s = list(hap[start:start + n])
    for p in rng.choice(n, size=errors, replace=False):
        s[int(p)] = _other(s[int(p)], int(rng.integers(1, 4)))
    return "".join(s), bytes((33 + rng.integers(q_lo, q_hi, n)).astype(np.uint8)).decode()


def likelihood_cases():
    rng = np.random.default_rng(401)
    ref = _bases(rng, 260)
    snp = ref[:120] + _other(ref[120]) + ref[121:]
    ins = ref[:60] + "TTG" + ref[60:]
    dele = ref[:180] + ref[184:]
    both = snp[:180] + snp[184:]
    out = []
    # every length around ceil(size * 0.02) and min(2.0, ...), from clean reads to reads past the threshold
    reads = []
    for n in (49, 50, 51, 100, 101, 200, 10, 1):
        for errors in (0, 1, 2, 3, 6):
            if errors <= n // 2:
                reads.append(_read_from(rng, (ref, snp, both)[len(reads) % 3], n, errors, 30, 41))
    out.append(("lengths", dict(reads=reads, haps=[ref, snp, ins, dele, both])))
    out.append(("one_haplotype", dict(reads=reads[:12], haps=[snp])))
    out.append(("two_haplotypes", dict(reads=reads[:12], haps=[ref, snp])))
    # unrelated reads of high quality: the fp32 pass underflows and the fp64 pass answers; every read is filtered
    junk = [(_bases(rng, n), "I" * n) for n in (60, 100, 150, 200)]
    out.append(("rescued_and_all_filtered", dict(reads=junk, haps=[ref, snp])))
    out.append(("rescued_among_good", dict(reads=reads[5:15] + junk[:2] + reads[15:20], haps=[ref, ins, dele])))
    # low qualities: the haplotypes stay close, the -4.5 cap changes nothing; high qualities: it does
    out.append(("low_quality", dict(reads=[_read_from(rng, both, 90, 1, 2, 8) for _ in range(8)], haps=[ref, snp, both])))
    out.append(("capped", dict(reads=[_read_from(rng, both, 150, 0, 40, 41, start=60) for _ in range(6)],
                               haps=[ref, snp, dele, both])))
    for k, r in enumerate(RW.regions(2, seed=402, n_reads=(20, 30))):
        out.append((f"region{k}", dict(reads=[(x[0].decode(), x[1].decode()) for x in r["reads"]],
                                       haps=[h.decode() for h in r["haps"]][:6])))
    return out


def likelihood_random(seed, n=24):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        ref = _bases(rng, int(rng.integers(40, 160)))
        haps = [ref]
        for _ in range(int(rng.integers(0, 4))):
            p = int(rng.integers(1, len(ref) - 5))
            haps.append([ref[:p] + _other(ref[p]) + ref[p + 1:], ref[:p] + "AC" + ref[p:], ref[:p] + ref[p + 3:]][int(rng.integers(0, 3))])
        reads = []
        for _ in range(int(rng.integers(1, 12))):
            h = haps[int(rng.integers(0, len(haps)))]
            ln = int(rng.integers(1, min(len(h), 200) + 1))
            reads.append(_read_from(rng, h, ln, int(rng.integers(0, min(ln, 8) // 2 + 1)), 2, 42)
                         if rng.random() < 0.9 else (_bases(rng, ln), "I" * ln))
        out.append((f"r{k}", dict(reads=reads, haps=haps)))
    return out


def threshold(read_len: int) -> float:
    """min(2.0, ceil(size * 0.02)) * -4.0 of intel_pairhmm.hpp:35-36, in doubles as written there."""
    return min(2.0, float(np.ceil(read_len * 0.02))) * -4.0


def normalize_cases():
    rng = np.random.default_rng(451)
    out = []
    lens = [1, 49, 50, 51, 99, 100, 101, 150, 200]
    # best exactly on the threshold (kept: the test is <), one step below (removed), one step above
    for name, step in (("on_threshold", 0), ("below_threshold", -1), ("above_threshold", 1)):
        rows = []
        for n in lens:
            t = threshold(n)
            best = t if step == 0 else float(np.nextafter(t, -np.inf if step < 0 else np.inf))
            rows.append([best - 6.0, best, best - 1.0])
        out.append((name, dict(read_len=lens, L=np.array(rows))))
    # the cap: values exactly on best - 4.5, one step either side, far below, -inf
    rows = []
    for best in (0.0, -0.125, -3.3, -7.9):
        cap = best + -4.5
        rows.append([best, cap, float(np.nextafter(cap, -np.inf)), float(np.nextafter(cap, np.inf)), -300.0, -np.inf])
    out.append(("cap", dict(read_len=[100] * 4, L=np.array(rows))))
    out.append(("one_haplotype", dict(read_len=lens, L=-rng.uniform(0, 10, (len(lens), 1)))))
    out.append(("two_haplotypes", dict(read_len=lens, L=-rng.uniform(0, 10, (len(lens), 2)))))
    out.append(("every_read_filtered", dict(read_len=[100] * 5, L=-rng.uniform(8.5, 30, (5, 3)))))
    out.append(("every_read_kept", dict(read_len=[100] * 5, L=-rng.uniform(0, 3, (5, 3)))))
    out.append(("one_read", dict(read_len=[77], L=np.array([[-1.0, -9.0]]))))
    out.append(("ties_and_signed_zero", dict(read_len=[60, 60, 60], L=np.array([[-2.0, -2.0], [0.0, -0.0], [-0.0, 0.0]]))))
    for k in range(3):
        G_L = G.region_matrix(rng, 30, 5 + k) * 1.7
        out.append((f"matrix{k}", dict(read_len=[int(x) for x in rng.integers(1, 201, 30)], L=G_L)))
    return out


def normalize_random(seed, n=200):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        nr, nh = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        L = -rng.gamma(2.0, 3.0, (nr, nh))
        lens = rng.integers(1, 201, nr)
        on = rng.random(nr) < 0.3   # rows whose best sits on, or a step off, its threshold
        for r in np.flatnonzero(on):
            t = threshold(int(lens[r]))
            L[r] = np.minimum(L[r], t - 0.5)
            L[r, int(rng.integers(0, nh))] = [t, float(np.nextafter(t, -np.inf)), float(np.nextafter(t, np.inf))][int(rng.integers(0, 3))]
        out.append((f"r{k}", dict(read_len=[int(x) for x in lens], L=L)))
    return out


# ---- genotype ------------------------------------------------------------------------

REF10 = b"ACGTACGTAC"   # window positions 0..9; position 4 is 'A'


def gt_region(haps, ref=REF10, pb=100, origin=None, reads=((90, 120),), L=None, seed=0):
    """haps: (bases, begin, cigar) after the reference path; L: rows per read, or seeded values in (-4, 0)."""
    hl = [dict(bases=ref, begin=0, cigar=f"{len(ref)}M")] + [dict(bases=b, begin=s, cigar=c) for b, s, c in haps]
    ob, oe = origin or (pb, pb + len(ref))
    if L is None:
        L = np.random.default_rng(seed).uniform(-4.0, 0.0, (len(reads), len(hl)))
    return dict(ref=ref, padded_begin=pb, origin_begin=ob, origin_end=oe, haps=hl,
                read_begin=np.array([r[0] for r in reads], np.int64), read_end=np.array([r[1] for r in reads], np.int64),
                L=np.ascontiguousarray(np.asarray(L, np.float64).reshape(len(reads), len(hl))))


SNP_T = (b"ACGTTCGTAC", 0, "10M")    # 104 A>T
SNP_C = (b"ACGTCCGTAC", 0, "10M")    # 104 A>C
INS_GG = (b"ACGTAGGCGTAC", 0, "5M2I5M")
DEL_3 = (b"ACGTAAC", 0, "5M3D2M")    # 104 ACGT>A
DEL_1 = (b"ACGTAGTAC", 0, "5M1D4M")  # 104 AC>A
BIG = np.finfo(np.float64).max


def quality_on_half(gt_oracle, target: float):
    """Two reads [0, -x] and [-x, 0] over a SNP site: 0/1 wins and the quality is
    round(-10 * (second - best)) with second falling as x grows. Returns the x
    nearest to target / 10 + 0.6 for which -10 * (second - best) is exactly
    `target` (a value on .5) in the arithmetic of gt_oracle (which the pins hold
    to the reference's bit for bit), or None."""
    amap, keep = np.array([0, 1], np.int32), np.array([0, 1], np.int32)

    def scaled(x):
        gl, _, _ = gt_oracle.site(np.array([[0.0, -x], [-x, 0.0]]), keep, amap, 2)
        top = sorted(gl)
        return -10 * (top[-2] - top[-1])

    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = (lo + hi) / 2
        if scaled(mid) < target:
            lo = mid
        else:
            hi = mid
    x = lo
    for _ in range(4000):
        if scaled(x) == target:
            return x
        x = float(np.nextafter(x, np.inf))
    return None


def genotype_cases(gt_oracle):
    import test_gt_regions as TG
    out = [(f"hand_{k}", TG.HAND[k][0]) for k in sorted(TG.HAND)]
    for k, reg in sorted(TG.shapes().items()):
        if len(reg["haps"]) <= 8 and len(reg["ref"]) <= 200:
            out.append((f"shape_{k}", reg))
    R = gt_region
    edge = [
        # one begin, different events on two haplotypes: a SNP and an insertion on the same anchor
        ("snp_and_insertion_at_one_begin", R([SNP_T, INS_GG])),
        ("two_snps_at_one_begin", R([SNP_T, SNP_C])),
        # REFs of 1, 2 and 4 bases at one site: every alt is extended to the longest
        ("refs_of_different_lengths", R([SNP_T, INS_GG, DEL_1, DEL_3], reads=((90, 120), (100, 106), (107, 120)))),
        # events one base before, on and one past either edge of the origin [103, 106)
        ("origin_edges", R([(b"ACCTACGTAC", 0, "10M"), (b"ACGAACGTAC", 0, "10M"), (b"ACGTAGGTAC", 0, "10M"),
                            (b"ACGTACCTAC", 0, "10M")], origin=(103, 106))),
        ("empty_origin", R([SNP_T], origin=(104, 104))),
        # a deletion that begins before the origin and spans a site inside it
        ("deletion_from_outside_spans_site", R([(b"ACGGTAC", 0, "3M3D4M"), (b"ACGTTCGTAC", 0, "10M")], origin=(104, 110))),
        ("leading_insertion_and_deletion", R([(b"GGACGTTCGTAC", 0, "2I10M"), (b"GTTCGTAC", 0, "2D8M")])),
        ("no_read_overlaps", R([SNP_T], reads=((0, 102), (107, 200), (300, 400)))),
        ("reads_touching_the_window", R([SNP_T], reads=((90, 102), (90, 103), (106, 120), (107, 120), (104, 105)))),
        ("minus_infinity", R([SNP_T, SNP_C], reads=((90, 120),) * 3,
                             L=[[-np.inf, -1.0, -2.0], [-1.0, -np.inf, -np.inf], [-np.inf, -np.inf, -np.inf]])),
        ("lowest", R([SNP_T, SNP_C], reads=((90, 120),) * 3, L=[[-BIG, -1.0, -2.0], [-1.0, -BIG, -BIG], [-BIG, -BIG, -BIG]])),
        ("lowest_one_read", R([SNP_T], reads=((90, 120),), L=[[-BIG, -BIG]])),
        # exact ties: equal columns give equal homozygous likelihoods; the > of :334 and the >= of :348 decide
        ("tie_equal_columns", R([SNP_T], reads=((90, 120),) * 2, L=[[-1.5, -1.5], [-0.25, -0.25]])),
        ("tie_three_alleles_no_reads", R([SNP_T, SNP_C], reads=())),
        ("tie_three_alleles_equal_columns", R([SNP_T, SNP_C], reads=((90, 120),), L=[[-2.0, -2.0, -2.0]])),
        ("tie_first_two", R([SNP_T, SNP_C], reads=((90, 120),), L=[[-1.0, -1.0, -4.0]])),
        ("tie_last_two", R([SNP_T, SNP_C], reads=((90, 120),), L=[[-4.0, -1.0, -1.0]])),
        ("zeros", R([SNP_T], reads=((90, 120),) * 4, L=np.zeros((4, 2)))),
        # sites at contig positions 0, 1 and 2
        ("contig_start", R([(b"CGTTACGTAC", 0, "10M"), (b"ACGTACGTAC", 0, "10M")], pb=0,
                           reads=((0, 50), (2, 9), (3, 9), (4, 9)))),
        ("contig_start_deletion", R([(b"AGTACGTAC", 0, "1M1D8M")], pb=0, reads=((0, 50), (4, 9), (5, 9)))),
        ("contig_position_2", R([(b"ACTTACGTAC", 0, "10M")], pb=0, reads=((0, 50), (0, 1), (1, 2), (5, 9), (4, 9)))),
        ("window_at_1", R([(b"CCGTACGTAC", 0, "10M")], pb=1, reads=((0, 50), (3, 9), (4, 9)))),
    ]
    out += edge
    for target in (0.5, 2.5, 49.5, 99.5):
        x = quality_on_half(gt_oracle, target)
        if x is not None:
            out.append((f"quality_on_{target}", R([SNP_T], reads=((90, 120),) * 2, L=[[0.0, -x], [-x, 0.0]])))
            y = float(np.nextafter(x, 0.0))
            out.append((f"quality_under_{target}", R([SNP_T], reads=((90, 120),) * 2, L=[[0.0, -y], [-y, 0.0]])))
    for k, reg in enumerate(G.regions(6, 120, 80, (3, 12), (12, 30), seed=73)):
        out.append((f"random{k}", reg))
    return out


def genotype_random(seed, n=40):
    out = [(f"r{k}", reg) for k, reg in enumerate(G.regions(n, 120, 80, (2, 14), (0, 30), seed=seed))]
    rng = np.random.default_rng(seed + 1)
    for k in range(n):   # windows at the contig's start, origin = the whole window
        ref = bytes(ACGT[int(x)] for x in rng.integers(0, 4, 12))
        haps = []
        for _ in range(int(rng.integers(1, 4))):
            alt = bytearray(ref)
            for p in rng.choice(5, size=int(rng.integers(1, 3)), replace=False):
                alt[int(p)] = ord(_other(chr(alt[int(p)]), int(rng.integers(1, 4))))
            haps.append((bytes(alt), 0, "12M"))
        nr = int(rng.integers(0, 6))
        rb = rng.integers(0, 8, nr)
        out.append((f"start{k}", gt_region(haps, ref=ref, pb=int(rng.integers(0, 3)),
                                           reads=tuple((int(b), int(b) + int(rng.integers(1, 9))) for b in rb), seed=seed + k)))
    return out


# ---- chain ---------------------------------------------------------------------------

def _chain_case(rng, window=200, origin=120, n_reads=30, pb=5000, p1=70):
    ref = _bases(rng, window)
    p2, p3 = 100, 130
    snp = ref[:p1] + _other(ref[p1]) + ref[p1 + 1:]
    dele = ref[:p2 + 1] + ref[p2 + 4:]
    ins = ref[:p3 + 1] + "GA" + ref[p3 + 1:]
    snp_del = snp[:p2 + 1] + snp[p2 + 4:]
    haps = [ref, snp, dele, ins, snp_del]
    truth = [haps[int(rng.integers(0, 5))], haps[int(rng.integers(0, 5))]]
    reads = []
    for k in range(n_reads):
        h = truth[k % 2]
        n = int(rng.integers(40, 90))
        st = 0 if k % 4 == 1 else int(rng.integers(0, len(h) - n + 1))
        seq, qual = _read_from(rng, h, n, int(rng.random() < 0.2), 25, 41, start=st)
        cigar, pos = f"{n}M", pb + st + 1
        if k % 7 == 3 and n > 30:   # a soft-clipped front of junk
            seq, cigar, pos = _bases(rng, 6) + seq[6:], f"6S{n - 6}M", pos + 6
        if k % 7 == 5 and n > 30:
            seq, cigar = seq[:-5] + _bases(rng, 5), f"{n - 5}M5S"
        reads.append(dict(flag=0x10 if k % 3 == 0 else 0, mapq=60, pos=pos, cigar=cigar, mate_same=1, seq=seq, qual=qual))
    if n_reads >= 12:
        reads[2]["mapq"], reads[4]["flag"], reads[6]["flag"], reads[8]["mate_same"] = 19, 0x400, 0x100, 0
        reads[10] = dict(flag=0, mapq=60, pos=pb + window - 9 + 1, cigar="40M", mate_same=1, seq=_bases(rng, 40), qual="I" * 40)
        if pb >= 30:   # thirty bases before the window
            reads[11] = dict(flag=0, mapq=60, pos=pb - 30 + 1, cigar="60M", mate_same=1, seq=_bases(rng, 30) + ref[:30],
                             qual="I" * 60)
    pad = (window - origin) // 2
    return dict(ref=ref, padded_begin=pb, origin_begin=pb + pad, origin_end=pb + pad + origin, haps=haps, reads=reads)


def chain_cases():
    rng = np.random.default_rng(501)
    out = [(f"region{k}", _chain_case(rng, n_reads=24 + 4 * k, pb=5000 + 300 * k)) for k in range(4)]
    for p1 in (1, 2):                                # a window at the contig's start with a SNP at position 1, 2
        c = _chain_case(rng, n_reads=20, pb=0, p1=p1)
        c["origin_begin"], c["haps"] = 0, c["haps"][:2]
        out.append((f"contig_start_snp_at_{p1}", c))
    out.append(("whole_contig", _whole_contig_case(rng)))
    c = _chain_case(rng, n_reads=16)
    for r in c["reads"]:
        r["mapq"] = 3
    out.append(("no_reads_left", c))
    c = _chain_case(rng, n_reads=16)
    c["haps"] = c["haps"][:1]
    out.append(("one_haplotype", c))
    return out


def _whole_contig_case(rng, length=200, n_reads=60):
    """A contig of one window (the default 245 + 85 cut at its end) whose reads begin
    at distinct positions, so that the contig caller picks every one of them."""
    c = _chain_case(rng, window=length, origin=length, n_reads=0, pb=0)
    ref, haps = c["ref"], c["haps"]
    truth = [haps[4], haps[3]]
    reads = []
    for k, st in enumerate(sorted(int(x) for x in rng.choice(length - 45, size=n_reads, replace=False))):
        h = truth[k % 2]
        n = min(int(rng.integers(50, 90)), len(h) - st)
        seq, qual = _read_from(rng, h, n, 0, 30, 41, start=st)
        # the read's begin on the contig: bases behind the deletion (ref 101..103) or the insertion (after 130) are shifted
        pos = st + (3 if st > 100 else 0) if h is haps[4] else st - (2 if st > 132 else 0)
        if h is haps[3] and 130 < st <= 132:
            continue   # begins inside the insertion
        reads.append(dict(flag=0x10 if k % 3 == 0 else 0, mapq=60, pos=pos + 1, cigar=f"{n}M", mate_same=1, seq=seq, qual=qual))
    seen, unique = set(), []
    for r in reads:
        if r["pos"] not in seen:
            seen.add(r["pos"])
            unique.append(r)
    return dict(c, origin_begin=0, origin_end=length, reads=unique)


def chain_random(seed, n=12):
    rng = np.random.default_rng(seed)
    return [(f"r{k}", _chain_case(rng, window=int(rng.integers(150, 260)), origin=100, n_reads=int(rng.integers(12, 40)),
                                  pb=int(rng.integers(0, 3)) * 4000)) for k in range(n)]


# ---- the reference's side, and the fixture's encoding ----------------------------------

STAGES = ("parse", "prepare", "align", "likelihoods", "normalize", "genotype", "chain")


def sam_text(reads) -> str:
    import oracle
    return "\n".join(oracle.sam_line(k, r["flag"], r["pos"], r["mapq"], r["cigar"], r["mate_same"], r["seq"], r["qual"])
                     for k, r in enumerate(reads))


def likelihood_sam(reads) -> str:
    """Reads of which only SEQ and QUAL matter."""
    import oracle
    return "\n".join(oracle.sam_line(k, 0, 1, 60, f"{len(s)}M", 1, s, q) for k, (s, q) in enumerate(reads))


def reference_output(stage: str, ref, x):
    """What the reference compiled in place (oracle.ChainReference) does with one
    input: a dict with threw = True, or threw = False and the stage's results."""
    import oracle
    try:
        if stage == "parse":
            out = ref.parse(x)
        elif stage == "prepare":
            out = dict(reads=ref.prepare(sam_text(x["reads"]), x["begin"], x["end"]))
        elif stage == "align":
            off, cigar = ref.align(x["ref"], x["alt"], tuple(x["params"]))
            out = dict(offset=off, cigar=cigar)
        elif stage == "likelihoods":
            out = ref.likelihoods(likelihood_sam(x["reads"]), x["haps"])
        elif stage == "normalize":
            kept, L = ref.normalize(x["L"], x["read_len"])
            out = dict(kept=kept, L=L)
        elif stage == "genotype":
            out = ref.genotype(x)
            out["whole_call_threw"] = out.pop("threw")
        elif stage == "chain":
            sam = sam_text(x["reads"])
            prepared = ref.prepare(sam, x["padded_begin"], x["padded_begin"] + len(x["ref"]))
            try:
                out = ref.chain(sam, x["haps"], x["ref"], x["padded_begin"], x["origin_begin"], x["origin_end"])
            except oracle.ReferenceThrew:
                return dict(threw=True, prepared=prepared)
            out["prepared"] = prepared
        else:
            raise KeyError(stage)
    except oracle.ReferenceThrew:
        return dict(threw=True)
    return dict(out, threw=False)


def encode(x):
    """Plain JSON data: doubles as their bits, bytes as latin-1 text, both tagged."""
    if isinstance(x, dict):
        return {str(k): encode(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if isinstance(x, bytes):
        return {"__bytes__": x.decode("latin-1")}
    if isinstance(x, np.ndarray):
        if x.dtype.kind == "f":
            a = np.ascontiguousarray(x, np.float64)
            return {"__f64__": list(a.shape), "bits": [int(v) for v in a.view(np.uint64).ravel()]}
        return {"__int__": list(x.shape), "values": [int(v) for v in x.ravel()]}
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, float):
        return {"__f64__": [], "bits": [int(np.float64(x).view(np.uint64))]}
    return x


def decode(x):
    if isinstance(x, list):
        return [decode(v) for v in x]
    if isinstance(x, dict):
        if "__bytes__" in x:
            return x["__bytes__"].encode("latin-1")
        if "__f64__" in x:
            a = np.array(x["bits"], np.uint64).view(np.float64).reshape(x["__f64__"])
            return a if x["__f64__"] else float(a)
        if "__int__" in x:
            return np.array(x["values"], np.int64).reshape(x["__int__"])
        return {k: decode(v) for k, v in x.items()}
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def load_fixture(path=None):
    """{stage: [{name, input, output}]} of tests/golden/chain_golden.npz."""
    import json
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_golden.npz")
    z = np.load(path, allow_pickle=False)
    return {stage: decode(json.loads(z[stage].tobytes().decode())) for stage in STAGES}


def prep_window(x):
    """A prepare input as hcprep.prep_reads takes it."""
    return dict(begin=x["begin"], end=x["end"],
                reads=[dict(flag=r["flag"], mapq=r["mapq"], pos=r["pos"], cigar=r["cigar"], mate_same=r["mate_same"],
                            seq_len=len(r["seq"])) for r in x["reads"]])
