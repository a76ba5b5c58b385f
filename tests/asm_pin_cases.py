"""Seeded cases of the assembler's pin to the reference compiled in place
(oracle/ref_asm_driver.cpp), their fixture and the census of the families.

A case is (name, region); a region is {"ref": bytes, "reads": [(bases, quals)]}
as in asm_cases.py. tests/golden/asm_golden.npz keeps every case's input and
the REFERENCE's record of it (oracle.AsmReference.assemble): status, kmer_size,
attempts, unique (k-mer counts), n_paths, haps [(bases, score)], source, sink,
edges [(from, to, last byte, count, is_ref, is_on_path, creation index)].

census(records) asserts, on the reference's records alone, the property every
family exists for; the fixture's generator refuses a fixture that fails it and
the suite repeats it on the committed file.
"""
from __future__ import annotations

import io
import json
import os
import random
import struct
import zipfile

import numpy as np

import asm_cases as AC
from asm_cases import rand_seq, region, sample_reads, snp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asm_golden.npz")

OK, NO_HAPLOTYPES, TOO_COMPLEX = 0, 1, 2
NOT_TRIED, SHORT_REF, TOO_MANY_KMERS, CYCLE, ACCEPTED = 0, 1, 2, 3, 4
MAX_PATHS = 65536

SEG_BORDERS = (64, 128, 192)
SEG_OFFSETS = (-26, -25, -1, 0, 1, 24, 25)
SEG_LENGTHS = (0, 1, 24, 25, 63, 64, 65, 127, 128, 129, 150, 192, 250, 300)
TIE_SIZES = (3, 4, 5, 6, 8)


def q(n, c=b"I"):
    return c * n


def both(bases):
    return (bases, q(len(bases)))


# ---- ties ---------------------------------------------------------------------------------

def snp_ladder(seed, n, spacing=40, copies=3, skew_at=()):
    """n SNPs `spacing` apart; per allele `copies` identical 56-base reads centred
    on the SNP. skew_at: at those SNPs the alternative allele is seen by one read fewer."""
    rng = random.Random(seed)
    ref = rand_seq(rng, spacing * (n - 1) + 60)
    reads = []
    for s in range(n):
        p = 30 + spacing * s
        alt = snp(ref, p)
        reads += [both(ref[p - 28:p + 28])] * copies
        reads += [both(alt[p - 28:p + 28])] * (copies - 1 if s in skew_at else copies)
    return region(ref, reads)


def tie_cases():
    out = [(f"ties_{n}", snp_ladder(300 + n, n)) for n in TIE_SIZES]
    # 2 : 3 support at two of the SNPs: 6 equal SNPs and 2 skewed ones put the cut inside a run of 40
    # mathematically equal scores whose neighbours on either side score differently
    out.append(("ties_8_skew", snp_ladder(320, 8, skew_at=(3, 5))))
    return out


# ---- the 2000 limit -----------------------------------------------------------------------

def limit_region(seed, last):
    rng = random.Random(seed)
    ref = rand_seq(rng, 400)
    reads = [both(rand_seq(rng, 101)) for _ in range(21)]
    return region(ref, reads + [both(last(rng))])


def limit_cases():
    def periodic(rng):   # 33 bases of period 8: 9 k-mers, the last is the first again
        unit = rand_seq(rng, 8)
        return (unit * 5)[:33]

    def broken(rng):     # the same read with its last base changed: 9 distinct k-mers
        r = periodic(rng)
        return snp(r, 32)
    return [("limit_2000", limit_region(401, lambda rng: rand_seq(rng, 31))),
            ("limit_2001", limit_region(401, lambda rng: rand_seq(rng, 32))),
            ("limit_dup_2000", limit_region(402, periodic)),
            ("limit_nodup_2002", limit_region(402, broken))]


# ---- high k -------------------------------------------------------------------------------

def noisy_region(seed, window, n_reads, read_len, err):
    rng = random.Random(seed)
    ref = rand_seq(rng, window)
    alt = snp(ref, window // 2)
    reads = []
    for j in range(n_reads):
        reads += sample_reads(rng, alt if j % 2 else ref, 1, rng.randint(*read_len), err=err)
    return region(ref, reads)


# (name, builder): found by a search over seeds and error rates against the compiled
# reference; census() holds them to the k they are named for.
HIGH_K = [
    ("high_k_65", lambda: noisy_region(*HIGH_K_ARGS[65])),
    ("high_k_75", lambda: AC.random_region(HIGH_K_ARGS[75], window=(200, 420), reads=(300, 420), err=0.02)),
    ("high_k_85", lambda: noisy_region(*HIGH_K_ARGS[85])),
    ("high_k_95", lambda: noisy_region(*HIGH_K_ARGS[95])),
    ("high_k_105", lambda: noisy_region(*HIGH_K_ARGS[105])),
]
HIGH_K_ARGS = {65: (9102, 400, 200, (60, 101), 0.01), 75: 8001, 85: (9101, 400, 250, (60, 101), 0.02),
               95: (9001, 400, 300, (90, 101), 0.03), 105: (9001, 400, 300, (101, 101), 0.03)}


def high_k_cases():
    return [(name, make()) for name, make in HIGH_K]


# ---- every attempt refused ----------------------------------------------------------------

def swapped_pair(x, y, copies=2):
    """Reads x+y and y+x: two different sequences that close a cycle x -> y -> x."""
    return [both(x + y)] * copies + [both(y + x)] * copies


def refused_cases():
    out = []
    rng = random.Random(501)   # 25, 35 too many k-mers; 45, 55 a cycle; the rest too short
    x, y = rand_seq(rng, 60), rand_seq(rng, 60)
    out.append(("refused_60_mixed", region(x, swapped_pair(x, y) + [both(rand_seq(rng, 101)) for _ in range(30)])))
    rng = random.Random(502)   # cycles only
    x, y = rand_seq(rng, 85), rand_seq(rng, 90)
    out.append(("refused_85_cycles", region(x, swapped_pair(x, y))))
    rng = random.Random(503)   # 25 .. 45 too many k-mers, 55 .. 105 a cycle
    x, y = rand_seq(rng, 110), rand_seq(rng, 106)
    out.append(("refused_110_mixed", region(x, swapped_pair(x, y, 3) + [both(rand_seq(rng, 101)) for _ in range(36)])))
    return out


# ---- the filter's third term and the cycle test -------------------------------------------

def filter_cases():
    rng = random.Random(601)
    ref = rand_seq(rng, 200)
    back = both(ref[120:150] + ref[60:90])
    x, y = rand_seq(rng, 30), rand_seq(rng, 30)
    from_sink = both(ref[170:200] + rand_seq(rng, 12) + ref[60:90])
    return [("filter_back_once", region(ref, [back])),
            ("filter_back_twice", region(ref, [back, back])),
            ("filter_cycle_off_window", region(ref, swapped_pair(x, y))),
            # the sink has no other out-edge, so the edge that leaves it passes with count 1
            ("filter_outdeg1_from_sink", region(ref, [from_sink])),
            # the same jump from the middle of the window: out-degree 2, filtered
            ("filter_outdeg2_from_middle", region(ref, [both(ref[140:170] + from_sink[0][30:])]))]


# ---- read shapes --------------------------------------------------------------------------

def seg_length_case():
    """Reads of every length of SEG_LENGTHS, longest first, centred on one long
    bubble: SNPs 20 apart over 120 bases, so every k-mer of the bubble is new and
    a read cut at a chunk border leaves the bubble in two parts. The reads of
    250 and 300 bases are longer than the window."""
    rng = random.Random(701)
    hap = rand_seq(rng, 330)
    alt = hap
    for p in range(100, 221, 20):
        alt = snp(alt, p)
    reads = []
    for n in reversed(SEG_LENGTHS):
        s = 165 - n // 2
        reads += [both(alt[s:s + n])] * 2
    return region(hap[50:280], reads)


def spoil(rng, bases, quals, p, how):
    b, qq = bytearray(bases), bytearray(quals)
    if how == 0:
        b[p] = ord("N")
    elif how == 1:
        qq[p] = 42
    else:
        qq[p] = 0x80 + rng.randrange(0x80)
    return bytes(b), bytes(qq)


def seg_edge_region(b, off, tail):
    """Reads of length p + 1 + tail that begin with the window, with their one
    unusable base at p = b + off, in two copies. The piece before p runs over
    every chunk border below p and carries SNPs 20 apart (one long bubble that
    comes back to the window 40 bases before p), so a piece cut or dropped at a
    border loses that haplotype. The piece behind p is `tail` (24 or 25) bases
    and holds one more SNP: only a kept piece (25) raises that branch's count.
    Two clean reads build that branch first."""
    rng = random.Random(7000 + 10 * b + off)
    p = b + off
    n = p + 1 + tail
    hap = rand_seq(rng, n + 40)
    at = p + 1 + 12                       # the SNP in the middle of the tail
    alt = snp(hap, at)
    for left in range(30, p - 40, 20):
        alt = snp(alt, left)
    clean = both(alt[at - 30:at + 30])
    bases, quals = spoil(rng, alt[:n], q(n), p, (b // 64 + off) % 3)
    return region(hap, [clean, clean, (bases, quals), (bases, quals)])


def seg_cases():
    out = [("seg_lengths", seg_length_case())]
    for b in SEG_BORDERS:
        for off in SEG_OFFSETS:
            for tail in (25, 24):
                out.append((f"seg_b{b}_p{off:+d}_tail{tail}", seg_edge_region(b, off, tail)))
    return out


# ---- degenerate windows -------------------------------------------------------------------

def degenerate_cases():
    out = []
    rng = random.Random(801)
    w = rand_seq(rng, 25)
    out.append(("window_is_one_25mer", region(w, [both(w)] * 2)))
    w, x, y = rand_seq(rng, 35), rand_seq(rng, 30), rand_seq(rng, 30)
    out.append(("window_is_one_35mer", region(w, swapped_pair(x, y) + [both(w)])))
    w = rand_seq(rng, 34)
    out.append(("window_34", region(w, [both(snp(w, 17))] * 2 + [both(w[3:])] * 2)))
    w = bytearray(rand_seq(rng, 150))
    w[30] = ord("N")
    w[85:95] = bytes(w[85:95]).lower()
    w = bytes(w)
    # set_ref does not filter: N and lower case are bytes like any other in the window; in a
    # read N ends a piece. Upper-case reads over the lower-case stretch and reads with A for
    # the N make two bubbles.
    out.append(("window_with_N_and_lower_case", region(w, [both(w[10:120])] * 2 + [both(w[40:140].upper())] * 2
                                                         + [both(w[0:80].replace(b"N", b"A"))] * 2)))
    a, b, c = rand_seq(rng, 40), rand_seq(rng, 40), rand_seq(rng, 40)
    w = a + b"A" * 62 + b + b"CA" * 31 + c
    out.append(("window_low_complexity", region(w, [both(a[10:] + b"A" * 70 + b[:20])] * 2
                                                + [both(b[15:] + b"CA" * 36 + c[:25])] * 2
                                                + [both(b"A" * 40), both(b"CA" * 20)])))
    w = rand_seq(rng, 150)
    out.append(("reads_all_unusable", region(w, [(snp(w, 70)[30:110], q(80, b"#")), (b"N" * 60, q(60)),
                                                  (snp(w, 70)[30:110], q(80, b"\xc9"))])))
    out.append(("reads_share_nothing", region(w, [both(rand_seq(rng, 90)) for _ in range(6)])))
    return out


# ---- tiny regions, and the large one that sizes a slot in front of them -------------------

def tiny_cases():
    """Windows of 25 to 60 bases with 0 to 4 reads. Their reads leave the window
    at a SNP and come back to it, so a vertex wrongly taken for a duplicate
    (workspace left over from another region) loses the alternative haplotype."""
    out = []
    rng = random.Random(901)
    # a SNP at p makes a bubble only with a whole k-mer on either side: 25 <= p <= length - 26
    for n, (wlen, n_reads) in enumerate([(25, 0), (30, 2), (38, 1), (44, 3), (51, 2), (52, 4), (54, 2), (55, 3), (56, 4),
                                         (58, 2), (60, 4), (60, 3)]):
        w = rand_seq(rng, wlen)
        alt = snp(w, 25 + (wlen - 51) // 2) if wlen >= 51 else w
        reads = [both(alt)] * min(n_reads, 2) + [both(w)] * max(0, n_reads - 2)
        out.append((f"tiny_{wlen}_{n_reads}_{n}", region(w, reads)))
    return out


def slot_sizer_case():
    """A large region whose window begins with a 60-base unit three times over:
    at every k the window's first k-mers are duplicates."""
    rng = random.Random(902)
    unit = rand_seq(rng, 60)
    w = unit * 3 + rand_seq(rng, 200)
    reads = []
    for _ in range(420):
        reads += sample_reads(rng, w, 1, 101, err=0.01)
    return [("slot_sizer", region(w, reads))]


# ---- more than 65 536 paths ---------------------------------------------------------------

def too_complex_cases():
    return [("bubbles_17", snp_ladder(1001, 17, spacing=30, copies=2))]


FAMILIES = dict(ties=tie_cases, limit=limit_cases, high_k=high_k_cases, refused=refused_cases, filter=filter_cases,
                seg=seg_cases, degenerate=degenerate_cases, tiny=tiny_cases, slot=slot_sizer_case,
                too_complex=too_complex_cases)


def all_cases():
    """[(family, name, region)]"""
    return [(fam, name, reg) for fam, make in FAMILIES.items() for name, reg in make()]


# ---- census -------------------------------------------------------------------------------

def score_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def result_key(rec):
    """What a wrong keep/drop decision on a read piece would change."""
    return (rec["attempts"], rec["n_paths"], [(h[0], score_bits(h[1])) for h in rec["haps"]],
            sorted(e[3] for e in rec["edges"]))


def census(recs):
    """recs: {name: the reference's record}. Asserts every family's property."""
    # ties
    for n in TIE_SIZES:
        r = recs[f"ties_{n}"]
        assert r["attempts"][0] == ACCEPTED and r["n_paths"] == 2 ** n, (n, r["attempts"], r["n_paths"])
        distinct = len({score_bits(h[1]) for h in r["haps"]})
        if n >= 5:
            assert r["n_paths"] > 16 and distinct < len(r["haps"]), (n, distinct)
    assert recs["ties_8"]["n_paths"] == 256 and len(recs["ties_8"]["haps"]) == 128
    skew = recs["ties_8_skew"]
    assert skew["n_paths"] == 256 and len(skew["haps"]) == 128
    assert len({score_bits(h[1]) for h in skew["haps"]}) > len({score_bits(h[1]) for h in recs["ties_8"]["haps"]})
    # the 2000 limit, on the driver's own count
    assert (recs["limit_2000"]["unique"][0], recs["limit_2000"]["attempts"][0]) == (2000, ACCEPTED)
    assert (recs["limit_2001"]["unique"][0], recs["limit_2001"]["attempts"][:2]) == (2001, [TOO_MANY_KMERS, ACCEPTED])
    assert (recs["limit_dup_2000"]["unique"][0], recs["limit_dup_2000"]["attempts"][0]) == (2000, ACCEPTED)
    assert (recs["limit_nodup_2002"]["unique"][0], recs["limit_nodup_2002"]["attempts"][0]) == (2002, TOO_MANY_KMERS)
    # high k
    ks = {recs[name]["kmer_size"] for name, _ in HIGH_K}
    assert len({k for k in ks if k > 55}) >= 4 and 105 in ks, ks
    for name, _ in HIGH_K:
        assert recs[name]["kmer_size"] == int(name.rsplit("_", 1)[1]), (name, recs[name]["kmer_size"])
    # every attempt refused
    refused = [recs[name] for name, _ in refused_cases()]
    assert all(r["status"] == NO_HAPLOTYPES and not r["haps"] and ACCEPTED not in r["attempts"] for r in refused)
    assert any({SHORT_REF, TOO_MANY_KMERS, CYCLE} <= set(r["attempts"]) for r in refused)
    assert all(CYCLE in r["attempts"] for r in refused)
    # filter
    assert recs["filter_back_once"]["attempts"][0] == ACCEPTED
    assert recs["filter_back_twice"]["attempts"][:2] == [CYCLE, ACCEPTED]
    assert recs["filter_cycle_off_window"]["attempts"][:2] == [CYCLE, ACCEPTED]
    assert recs["filter_outdeg1_from_sink"]["attempts"][0] == CYCLE
    assert recs["filter_outdeg2_from_middle"]["attempts"][0] == ACCEPTED
    # read shapes: a piece of 25 is kept and one of 24 dropped, and that shows
    for b in SEG_BORDERS:
        for off in SEG_OFFSETS:
            keep, drop = recs[f"seg_b{b}_p{off:+d}_tail25"], recs[f"seg_b{b}_p{off:+d}_tail24"]
            assert keep["status"] == OK and drop["status"] == OK and keep["kmer_size"] == drop["kmer_size"] == 25
            assert len(keep["haps"]) == len(drop["haps"]) == (4 if b + off - 40 > 30 else 2), (b, off)
            assert [score_bits(h[1]) for h in keep["haps"]] != [score_bits(h[1]) for h in drop["haps"]], (b, off)
    lengths = recs["seg_lengths"]
    assert lengths["status"] == OK and len(lengths["haps"]) >= 2
    # degenerate windows
    for name in ("window_is_one_25mer", "window_is_one_35mer"):
        r = recs[name]
        assert r["status"] == OK and r["source"] == r["sink"] and r["n_paths"] == 1 and len(r["haps"][0][0]) == r["kmer_size"]
    assert recs["window_is_one_35mer"]["attempts"][:2] == [CYCLE, ACCEPTED]
    assert recs["window_34"]["attempts"][:2] == [ACCEPTED, NOT_TRIED] and len(recs["window_34"]["haps"]) == 1
    odd = recs["window_with_N_and_lower_case"]
    assert odd["status"] == OK and any(b"N" in h[0] for h in odd["haps"]) and any(h[0] != h[0].upper() for h in odd["haps"])
    assert len(odd["haps"]) >= 2
    assert recs["window_low_complexity"]["status"] == OK
    for name in ("reads_all_unusable", "reads_share_nothing"):
        assert recs[name]["n_paths"] == 1 and recs[name]["attempts"][0] == ACCEPTED
    assert len(recs["reads_all_unusable"]["edges"]) < len(recs["reads_share_nothing"]["edges"])
    # tiny regions: the alternative haplotype is there where two reads carry it
    tiny = {name: recs[name] for name, _ in tiny_cases()}
    assert len(tiny) >= 12 and all(r["status"] == OK for r in tiny.values())
    assert sum(len(r["haps"]) == 2 for r in tiny.values()) >= 8
    assert recs["slot_sizer"]["status"] == OK
    # more than 65 536 paths
    assert recs["bubbles_17"]["n_paths"] == 2 ** 17 and len(recs["bubbles_17"]["haps"]) == 128


# ---- the fixture --------------------------------------------------------------------------

def _s(b: bytes) -> str:
    return b.decode("latin-1")


def _b(s: str) -> bytes:
    return s.encode("latin-1")


def encode(rows):
    """[(family, name, region, record)] as JSON-able data: bytes as latin-1 text, scores as bits."""
    out = []
    for fam, name, reg, rec in rows:
        out.append(dict(family=fam, name=name, ref=_s(reg["ref"]), reads=[[_s(b), _s(qq)] for b, qq in reg["reads"]],
                        status=rec["status"], kmer_size=rec["kmer_size"], attempts=rec["attempts"], unique=rec["unique"],
                        n_paths=rec["n_paths"], haps=[[_s(h[0]), score_bits(h[1])] for h in rec["haps"]],
                        source=rec["source"], sink=rec["sink"], edges=[list(e) for e in rec["edges"]]))
    return out


def decode(data):
    """The inverse of encode: [dict(family, name, region, record)]."""
    out = []
    for d in data:
        rec = dict(status=d["status"], kmer_size=d["kmer_size"], attempts=d["attempts"], unique=d["unique"],
                   n_paths=d["n_paths"],
                   haps=[(_b(h), struct.unpack("<d", struct.pack("<Q", bits))[0]) for h, bits in d["haps"]],
                   source=d["source"], sink=d["sink"], edges=[tuple(e) for e in d["edges"]])
        out.append(dict(family=d["family"], name=d["name"],
                        region=region(_b(d["ref"]), [(_b(b), _b(qq)) for b, qq in d["reads"]]), record=rec))
    return out


def write_fixture(rows, path=GOLDEN):
    blob = json.dumps(encode(rows), sort_keys=True, separators=(",", ":")).encode()
    buf = io.BytesIO()
    np.lib.format.write_array(buf, np.frombuffer(blob, np.uint8), allow_pickle=False)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        z.writestr(zipfile.ZipInfo("cases.npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                   compress_type=zipfile.ZIP_DEFLATED, compresslevel=9)


def load_fixture(path=GOLDEN):
    with np.load(path) as z:
        return decode(json.loads(z["cases"].tobytes().decode()))


# ---- comparisons --------------------------------------------------------------------------

def row(name, when, reference, library, basis):
    return dict(name=name, when=when, reference=reference, library=library, basis=basis)


# The one list of inputs on which the library (and with it the restatement) does
# not do what the reference does, in the form of test_ref_pins.DEVIATIONS.
DEVIATIONS = [
    row("more than 65 536 paths",
        lambda rec: rec["n_paths"] > MAX_PATHS,
        "path_finder enumerates every path, however many, and keeps the best 128",
        "status HC_ASM_TOO_COMPLEX, n_paths HC_ASM_MAX_PATHS + 1, no haplotypes",
        "include/hc_asm.h: 'an attempt with more than HC_ASM_MAX_PATHS paths ends the region as HC_ASM_TOO_COMPLEX'"),
]


def library_expectation(rec):
    """(what the library must give on a case with this reference record, in the
    layout of asm_util.assert_same; the table's rows that apply)."""
    rows = [r for r in DEVIATIONS if r["when"](rec)]
    exp = dict(rec, graph=on_path_graph(rec))
    if rows:
        exp.update(status=TOO_COMPLEX, n_paths=MAX_PATHS + 1, haps=[])
    return exp, rows


def same_as_reference(got, rec):
    """Does a library result equal the reference's record, order and score bits included?"""
    return ((got["attempts"], got["status"], got["kmer_size"], got["n_paths"]) ==
            (rec["attempts"], rec["status"], rec["kmer_size"], rec["n_paths"]) and
            [(h[0], score_bits(h[1])) for h in got["haps"]] == [(h[0], score_bits(h[1])) for h in rec["haps"]])


def check_table(results):
    """results: [(name, reference record, library result, compare)] where compare(got, exp)
    asserts equality. Holds every case to the reference, or to its table row, and
    the table to the cases: fails on a deviation outside the table, on a row that
    no longer deviates and on a row no case meets."""
    met = set()
    for name, rec, got, compare in results:
        exp, rows = library_expectation(rec)
        compare(got, exp, name)
        if rows:
            assert not same_as_reference(got, rec), f"{name}: row {rows[0]['name']!r} no longer deviates"
            met.update(r["name"] for r in rows)
    missing = {r["name"] for r in DEVIATIONS} - met
    assert not missing, f"table rows that no case meets: {sorted(missing)}"


def runs(haps):
    """[(score bits, [bases])] of consecutive haplotypes with equal score bits."""
    out = []
    for bases, score in haps:
        bits = score_bits(score)
        if out and out[-1][0] == bits:
            out[-1][1].append(bases)
        else:
            out.append((bits, [bases]))
    return out


def assert_equal_up_to_ties(kept, all_sorted, ref_haps, n_paths, what=""):
    """The restatement (stable sort: `kept` after the cut, `all_sorted` before it)
    against the reference's haplotypes: the sequence of score bits is the same;
    within a run of equal score bits the members are the same as a multiset, in
    any order; where such a run is the last and the cut fell (n_paths above the
    number kept), the reference's members of it are among the restatement's
    members of the whole run. Outside runs that is exact equality."""
    assert [score_bits(h[1]) for h in kept] == [score_bits(h[1]) for h in ref_haps], what
    mine, theirs = runs(kept), runs(ref_haps)
    assert [b for b, _ in mine] == [b for b, _ in theirs], what
    cut = n_paths > len(ref_haps)
    for k, ((bits, a), (_, b)) in enumerate(zip(mine, theirs)):
        if cut and k == len(mine) - 1:
            pool = sorted(h[0] for h in all_sorted if score_bits(h[1]) == bits)
            for bases in b:
                assert bases in pool, (what, "a haplotype of the last run that is no path of that score")
                pool.remove(bases)
        else:
            assert sorted(a) == sorted(b), (what, k)


def slot_order(fixture, n, n_slots):
    """n cases for a call in which workspace slices are used again (slice b runs
    regions b, b + n_slots, ..): a dozen of the smallest cases in turn, every
    50th one of the largest, and two large ones as second regions of slices
    whose first was tiny. So small follows large in a slice and the reverse."""
    by_name = {c["name"]: c for c in fixture}
    tiny = [c for c in fixture if c["family"] == "tiny"]
    large = [by_name[name] for name in ("slot_sizer", "high_k_75", "window_low_complexity")]
    assert len(tiny) >= 12
    assert all(25 <= len(c["region"]["ref"]) <= 60 and len(c["region"]["reads"]) <= 4 for c in tiny)
    second = {n_slots + 5: large[0], n_slots + 20: large[1]}
    order = [large[(k // 50) % 3] if k % 50 == 0 else second.get(k, tiny[k % len(tiny)]) for k in range(n)]
    assert order[0] is large[0] and order[5]["family"] == "tiny" and (n <= n_slots or order[n_slots]["family"] == "tiny")
    return order


def on_path_graph(rec):
    """The reference's on-path edges in asm_util.canon_graph's layout."""
    return [(u, v, base, count, is_ref, seq) for u, v, base, count, is_ref, on_path, seq in rec["edges"] if on_path]
