"""Inputs shared by the tests of the SAM parser and the contig caller
(test_sam_restate.py, test_sam_host.py, test_gpu_sam.py, test_gpu_contig.py,
test_gpu_contig_dropin.py) and their expected side from the restatement
(sam_restate.py), computed once.

texts(): the parse grid and its companions. The grid has a line of every length
from 1 to 700 bytes: the shortest line that is a record has 21 bytes
("a 0 b 1 0 * = 0 0 * *"), so the lines of 1 to 20 bytes are blank lines (which
have no record) and those of 21 to 700 are records; lines of 1 to 20 bytes that
hold a token are errors and are among the error texts, one per length. Newlines
and token starts fall on every offset modulo 64 and modulo 16
(test_sam_restate.test_grid_covers_every_offset checks all of that).
chunk_edges and chunk_edges_crlf put newlines on the last and the first byte of
the line scan's 1 KiB chunks; many_lines has more than 4096 lines in more than
4096 chunks, so that every scan of the parser runs over several tiles.

error_texts(): one defective text per syntax error, each alone and after the
grid with a second, later error.

contig(): a contig of 13 windows, 12 x 245 bases and a 47-base tail, with its
reads as SAM text. One read per filter reason begins in the origin of every
window but 8 (which has no reads at all) and 12 (the 47-base tail, where no
read begins: reads are at least 30 bases long).

flat_contig(): 9 000 bases without variants and reads of 50 bases, for the
position scan over several tiles (37 windows) and, tiled 2 + 2 x 1, the window
scan over several tiles (4 500 windows).
"""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np

import call_cases as CC
import sam_restate as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("line_no", "line", "seq_off", "qual_off", "seq_len", "qual_len", "pos", "cigar", "n_cigar", "flag", "mapq",
          "mate_same_contig", "defect")
ERROR_CODES = {1: "fields", 2: "FLAG", 3: "POS", 4: "MAPQ", 5: "CIGAR", 6: "PNEXT", 7: "TLEN"}
# what the library's message says about each (include/hc_sam.h names the field)
ERROR_TEXT = dict(fields="fewer than 11 fields", FLAG="FLAG is not", POS="POS is not", MAPQ="MAPQ is not",
                  CIGAR="CIGAR is neither", PNEXT="PNEXT is not", TLEN="TLEN is not")
HEADER = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrT\tLN:2987\n@PG\tID:sam_cases\n"


def line(qname="q", flag=0, rname="chrT", pos=100, mapq=60, cigar=None, rnext="=", pnext=0, tlen=0, seq="ACGT",
         qual=None, sep="\t", tags=()):
    cigar = f"{len(seq)}M" if cigar is None else cigar
    qual = "I" * len(seq) if qual is None else qual
    return sep.join(str(x) for x in (qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual) + tuple(tags))


def _seq(n, k=0):
    return ("ACGTTGCA" * (n // 8 + 2))[k % 8:k % 8 + n]


def line_of_length(n, k=0, tail=""):
    """A record of exactly n >= 60 bytes (`tail` included), its SEQ about half of it."""
    short = line(qname="r", pos=1000 + k, seq=_seq((n - len(tail) - 44) // 2, k), flag=(0, 16, 99, 147)[k % 4]) + tail
    out = "r" * (n - len(short)) + short
    assert len(out) == n and n >= len(short)
    return out


@functools.lru_cache(maxsize=None)
def grid_lines():
    out = ["a 0 b 1 0 * = 0 0 * *"]
    out += [(" \t\r\v\f" * 4)[:n] for n in range(1, 21)]                                  # blank lines of 1 .. 20
    out += ["a" * n + " 0 b 1 0 * = 0 0 * *" for n in range(2, 15)]                     # 22 .. 34
    out += [line(qname="q" * n, seq="ACGT") for n in range(1, 66)]                      # every length 34 .. 98
    out += [line_of_length(n, n) for n in range(99, 701)]
    out += [line(qname=f"s{n}", pos=n + 1, seq=_seq(11 + (n * 7) % 45, n)) for n in range(300)]   # more starts and ends
    out += [
        line(qname="ops", cigar="1M2I3D4N5S6H7P8=9X", seq=_seq(25)),
        line(qname="long_cigar", cigar="1M1I" * 100, seq=_seq(200)),
        line(qname="max_len", cigar="268435455M", seq=_seq(9)),
        line(qname="max_len_d", cigar="268435455D4M268435455N", seq="ACGT"),
        line(qname="zeros", flag="000016", pos="0000000100", mapq="060", cigar="0004M", pnext="00", tlen="-000"),
        line(qname="extremes", flag=65535, pos=4294967295, mapq=65535, pnext=4294967295, tlen=-2147483648),
        line(qname="tlen_max", tlen=2147483647),
        line(qname="stars", cigar="*", seq="*", qual="*"),
        line(qname="spaces", sep=" "),
        line(qname="mixed", sep=" \t\v\f "),
        line(qname="crlf") + "\r",
        "",
        "   \t ",
        "\r",
        "  " + line(qname="indented") + "  ",
        line(qname="@late"),          # a later line that starts with '@' is an alignment line
        line(qname="@CO", sep=" "),
        line(qname="tags", tags=("NM:i:0", "XX:Z:hello world", "-1", "5Z")),
        line(qname="other_contig", rname="chrOther", rnext="chrOther"),
        line(qname="rnext_eq_eq", rnext="=="),
        line(qname="defect_pos", pos=0),
        line(qname="defect_pos_and_more", pos=0, cigar="*", qual="II"),
        line(qname="defect_no_cigar", cigar="*"),
        line(qname="defect_cigar_length", cigar="3M"),
        line(qname="defect_cigar_length_clip", cigar="4M2H1D", seq="ACGTA"),
        line(qname="defect_qual_length", qual="III"),
        line(qname="defect_too_long", seq=_seq(65537)),
        line(qname="just_fits", seq=_seq(65536)),
        line(qname="last_line_without_newline", seq=_seq(70)),
    ]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def texts():
    grid = (HEADER + "\n".join(grid_lines())).encode("latin-1")
    one = line(qname="only").encode()
    return dict(grid=grid, grid_newline=grid + b"\n", grid_crlf=grid.replace(b"\n", b"\r\n"),
                no_header=b"\n".join(x.encode("latin-1") for x in grid_lines()[:40]) + b"\n",
                header_only=HEADER.encode(), header_only_open=HEADER.encode()[:-1], empty=b"", newline=b"\n",
                blank_only=b"\n \n\t\r\n\n", one_line=one, one_line_newline=one + b"\n",
                one_after_blank=b"\n" + one,
                # newlines at 1023, 2047, 3072 (a chunk's first byte), 4095, then a line across a whole chunk
                chunk_edges="".join(line_of_length(n, n) + "\n" for n in (1023, 1023, 1024, 1022, 2500, 70)).encode(),
                # "\r\n" across the edge: '\r' at 1023 and '\n' at 1024, then '\n' at 2047
                chunk_edges_crlf="".join(line_of_length(n, n, "\r") + "\n" for n in (1024, 1022, 100)).encode(),
                many_lines=(HEADER + "".join(line_of_length(440 + (n * 37) % 90, n) + "\n" for n in range(9000))).encode())


@functools.lru_cache(maxsize=None)
def error_lines():
    """(name, the defective line, the field the message must name)."""
    return (
        ("one_byte", "x", "fields"),
        ("ten_fields", " ".join(line(sep=" ").split(" ")[:10]), "fields"),
        ("flag_sign", line(flag="-1"), "FLAG"),
        ("flag_overflow", line(flag=65536), "FLAG"),
        ("flag_letters", line(flag="12a"), "FLAG"),
        ("pos_plus", line(pos="+1"), "POS"),
        ("pos_overflow", line(pos=4294967296), "POS"),
        ("pos_huge", line(pos="9" * 40), "POS"),
        ("mapq_letter", line(mapq="6o"), "MAPQ"),
        ("mapq_hex", line(mapq="0x10"), "MAPQ"),
        ("cigar_operator", line(cigar="4Z"), "CIGAR"),
        ("cigar_lower_case", line(cigar="4m"), "CIGAR"),
        ("cigar_no_digits", line(cigar="M4M"), "CIGAR"),
        ("cigar_no_digits_inside", line(cigar="2MM2M"), "CIGAR"),
        ("cigar_trailing_digits", line(cigar="4M3"), "CIGAR"),
        ("cigar_digits_only", line(cigar="4"), "CIGAR"),
        ("cigar_star_star", line(cigar="**"), "CIGAR"),
        ("cigar_length", line(cigar="268435456M"), "CIGAR"),
        ("cigar_length_huge", line(cigar="9" * 30 + "M"), "CIGAR"),
        ("pnext_sign", line(pnext="-5"), "PNEXT"),
        ("tlen_overflow", line(tlen=2147483648), "TLEN"),
        ("tlen_underflow", line(tlen=-2147483649), "TLEN"),
        ("tlen_plus", line(tlen="+7"), "TLEN"),
        ("tlen_minus_only", line(tlen="-"), "TLEN"),
        ("tlen_float", line(tlen="1.5"), "TLEN"),
        *[(f"short_{n}", ("xy z" * 5)[:n].strip().ljust(n, "x"), "fields") for n in range(1, 21)],
        ("fields_before_flag", line(flag="zz", sep=" ").rsplit(" ", 3)[0], "fields"),
        ("flag_before_cigar", line(flag="zz", cigar="4Z"), "FLAG"),
    )


@functools.lru_cache(maxsize=None)
def error_texts():
    """(name, text, the 1-based line the message must name, the field). Each
    defective line alone under the header, and after the grid with a second,
    different error three lines further down."""
    out = []
    n_header = HEADER.count("\n")
    grid = texts()["grid_newline"].decode("latin-1")
    n_grid = grid.count("\n")
    lines = error_lines()
    for k, (name, bad, field) in enumerate(lines):
        out.append((name, (HEADER + bad + "\n").encode("latin-1"), n_header + 1, field))
        if name.startswith("short_"):
            continue
        later = lines[(k + 5) % len(lines)][1]
        text = grid + line() + "\n" + bad + "\n" + line() + "\n\n" + later + "\n" + line()
        out.append((name + "_after_grid", text.encode("latin-1"), n_grid + 2, field))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """The restatement's parse of texts()[name]."""
    return SR.load_all_reads(texts()[name])


def record_rows(parsed):
    """The restatement's (or hccontig's) records as tuples in FIELDS order."""
    recs = parsed["records"]
    if isinstance(recs, np.ndarray):
        return [tuple(int(parsed["line_no"][k]) if f == "line_no" else int(r[f]) for f in FIELDS) for k, r in enumerate(recs)]
    return [tuple(int(r[f]) for f in FIELDS) for r in recs]


def assert_same_parse(got, exp, tag=""):
    """Records field for field, the pool word for word, the header's length."""
    g, e = record_rows(got), record_rows(exp)
    assert len(g) == len(e), (tag, len(g), len(e))
    for k, (a, b) in enumerate(zip(g, e)):
        assert a == b, (tag, k, dict(zip(FIELDS, a)), dict(zip(FIELDS, b)))
    assert [int(x) for x in got["pool"]] == [int(x) for x in exp["pool"]], tag
    assert got["n_header_lines"] == exp["n_header_lines"], tag


# ---- tests/cpp/sam_host_main.cpp ---------------------------------------------------

def build_host_main(tmp_path):
    exe = tmp_path / "sam_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSAMX_HOST_ONLY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sam_host_main.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def parse_host_output(text):
    """"H n_header n_records n_words", one line per record in FIELDS order, "P word...": as load_all_reads gives it."""
    rows = text.splitlines()
    tok = rows[0].split()
    assert tok[0] == "H"
    n_header, n_rec, n_words = int(tok[1]), int(tok[2]), int(tok[3])
    recs = [dict(zip(FIELDS, (int(x) for x in rows[1 + k].split()))) for k in range(n_rec)]
    pool = [int(x) for x in rows[1 + n_rec].split()[1:]]
    assert rows[1 + n_rec].split()[0] == "P" and len(pool) == n_words
    return dict(records=recs, pool=pool, n_header_lines=n_header)


# ---- the contig ----------------------------------------------------------------------

REGION, PADDING = 245, 85
N_WINDOWS, TAIL = 13, 47
REF_LEN = 12 * REGION + TAIL
CONTIG = "chrT"
NO_VARIANT_WINDOW, NO_READS_WINDOW = 4, 8
CONTIG_SEED = 20261020


def _plant(rng, ref):
    """The variant haplotype over the whole contig, as call_cases._variant_hap
    plants it per window: per haplotype base its contig position (-1: inserted).
    Variants lie inside origins, at least 45 apart, none in windows 4, 8 and 12."""
    hap, where, p = bytearray(), [], 0
    for w in range(12):
        if w in (NO_VARIANT_WINDOW, NO_READS_WINDOW):
            continue
        # window 4's reads begin in [895, 1310) and end before 1411: its neighbours' variants stay outside that
        lo = w * REGION + (195 if w == NO_VARIANT_WINDOW + 1 else 20)
        sites = [lo + int(rng.integers(0, 20))]
        if rng.random() < 0.6 and w != NO_VARIANT_WINDOW + 1:
            sites.append(sites[0] + 60 + int(rng.integers(0, 40 if w == NO_VARIANT_WINDOW - 1 else 100)))
        for k, v in enumerate(sites):
            hap += ref[p:v]
            where += range(p, v)
            kind = "D" if (w == 1 and k == 0) else "SDI"[int(rng.integers(0, 3))]
            hap.append(ref[v] if kind != "S" else CC.ACGT[(CC.ACGT.index(ref[v]) + 1 + int(rng.integers(0, 3))) % 4])
            where.append(v)
            p = v + 1
            if kind == "D":
                p += int(rng.integers(1, 6))
            elif kind == "I":
                ins = CC._bases(rng, int(rng.integers(1, 5)))
                hap += ins
                where += [-1] * len(ins)
    hap += ref[p:]
    where += range(p, len(ref))
    return bytes(hap), where


def _sam_line(name, r, rname=CONTIG):
    return line(qname=name, flag=r["flag"], rname=rname, pos=r["pos"], mapq=r["mapq"], cigar=r["cigar"],
                rnext="=" if r["mate_same"] else "chrOther", pnext=r["pos"] + 150, tlen=250,
                seq=r["bases"].decode(), qual=r["quals"].decode())


@functools.lru_cache(maxsize=None)
def contig():
    """dict(ref, reads = [(name, read dict as call_cases gives it, rname)] in
    generation order, sam = the reads in a shuffled order with a header, and
    sam_reshuffled = another order that keeps every position's reads in their order)."""
    rng = np.random.default_rng(CONTIG_SEED)
    ref = CC._bases(rng, REF_LEN)
    hap, where = _plant(rng, ref)
    sources = [(ref, list(range(REF_LEN))), (hap, where)]
    quiet = (NO_READS_WINDOW * REGION - PADDING, (NO_READS_WINDOW + 1) * REGION + PADDING)   # no read begins here
    reads = []
    for start in range(0, REF_LEN - 30):
        for _ in range(int(rng.choice([0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 3]))):
            h, wh = sources[int(rng.random() < 0.5)]
            length = min(int(rng.integers(60, 102)), len(h) - start)
            if start >= len(h) - 30:
                continue
            r = CC._read(rng, h, wh, 0, start, length, 0.12)
            if quiet[0] <= r["pos"] - 1 < quiet[1]:
                continue
            reads.append(r)
    for w in range(N_WINDOWS - 1):   # one read per filter reason that begins in the window's origin
        if w == NO_READS_WINDOW:
            continue
        mine = [r for r in reads if w * REGION <= r["pos"] - 1 < (w + 1) * REGION and r["mapq"] == 60 and r["mate_same"]
                and not r["flag"] & 0x500]
        mine[3]["mapq"] = 19
        mine[7]["flag"] |= 0x400
        mine[11]["flag"] |= 0x100
        mine[15]["mate_same"] = 0
        # nine bases inside the window's padded end: removed for length there, a whole read one window on
        at = (w + 1) * REGION + PADDING - 9
        if at + 60 <= REF_LEN and not quiet[0] <= at < quiet[1]:
            reads.append(dict(flag=0, mapq=60, pos=at + 1, cigar="60M", mate_same=1, seq_len=60, bases=ref[at:at + 60],
                              quals=b"I" * 60))
    named = [(f"read{k}", r, "chrOther" if k % 97 == 0 else CONTIG) for k, r in enumerate(reads)]
    order = rng.permutation(len(named))
    sam = HEADER + "".join(_sam_line(*named[k]) + "\n" for k in order)
    # the same lists per position, the positions interleaved differently
    by_pos = {}
    for k in order:
        by_pos.setdefault(named[k][1]["pos"], []).append(k)
    keys = list(by_pos)
    again = []
    while keys:
        pos = keys[int(rng.integers(0, len(keys)))]
        again.append(by_pos[pos].pop(0))
        if not by_pos[pos]:
            keys.remove(pos)
    sam2 = HEADER + "".join(_sam_line(*named[k]) + "\n" for k in again)
    assert again != list(order)
    return dict(ref=ref, reads=named, sam=sam.encode(), sam_reshuffled=sam2.encode())


@functools.lru_cache(maxsize=None)
def flat_contig():
    """dict(ref, sam, sam_mapq0): 9 000 bases, about one read of 50 bases beginning
    per position (0, 1 or 2), unsorted; sam_mapq0 is the same file with MAPQ 0."""
    rng = np.random.default_rng(CONTIG_SEED + 1)
    ref = CC._bases(rng, 9000)
    starts = np.repeat(np.arange(9000 - 50), rng.integers(0, 3, 9000 - 50))
    rng.shuffle(starts)
    out = {}
    for key, mapq in (("sam", 60), ("sam_mapq0", 0)):
        out[key] = (HEADER + "".join(line(qname=f"f{k}", pos=int(s) + 1, mapq=mapq, seq=ref[s:s + 50].decode(), flag=99) + "\n"
                                     for k, s in enumerate(starts))).encode()
    return dict(ref=ref, **out)


def restated_windows(sam: bytes, ref: bytes, pick="seeded", seed=0, skip_unplaced=False, region=REGION, padding=PADDING):
    """The restatement's side of a contig call: (parse, per window a dict of the
    bounds, the reference slice, `picked` record indices and the window as
    hccall.call_windows takes it). The chain's origin is cut at the contig's end
    (hc_gt.h refuses an origin past the window's reference; no event lies there)."""
    parsed = SR.load_all_reads(sam)
    recs, pool = parsed["records"], parsed["pool"]
    rmap = SR.reads_map(recs, len(ref), skip_unplaced)
    picked = SR.picks(rmap, len(ref), region, padding, SR.pick_fn(pick, seed))
    text = sam.decode("latin-1")
    out = []
    for (pb, pe, ob, oe), idx in zip(SR.window_bounds(len(ref), region, padding), picked):
        slice_ = ref[pb:pe]
        reads = []
        for k in idx:
            r = recs[k]
            at = r["line"]
            reads.append(dict(flag=r["flag"], mapq=r["mapq"], pos=r["pos"],
                              cigar=np.array(pool[r["cigar"]:r["cigar"] + r["n_cigar"]], np.uint32),
                              mate_same=r["mate_same_contig"], seq_len=r["seq_len"],
                              bases=text[at + r["seq_off"]:at + r["seq_off"] + r["seq_len"]].encode("latin-1"),
                              quals=text[at + r["qual_off"]:at + r["qual_off"] + r["qual_len"]].encode("latin-1")))
        out.append(dict(padded_begin=pb, padded_end=pe, origin_begin=ob, origin_end=oe, ref_len=len(slice_), picked=idx,
                        call=dict(ref=slice_, padded_begin=pb, padded_end=pe, origin_begin=ob,
                                  origin_end=min(oe, len(ref)), reads=reads)))
    return parsed, out
