"""A literal, sequential restatement of lines 93-94 of the reference's
HaplotypeCaller::call_region: filter_reads and hard_clip_reads
(haplotypecaller.hpp:52-81) over utils/read_filter.hpp, utils/read_clipper.hpp:
32-91, sam/sam.hpp:69-72 and sam/cigar.hpp:92-111. It works on string slices
and a list of CIGAR elements, statement by statement as the headers do, and
shares no code with the library (no views, no packed words, no bit masks).

Integer widths: POS is uint32 and wraps as such; everything else is size_t and
wraps at 2^64. std::string::substr(pos, n) is restated with its own rules: pos
beyond size() throws, n is cut to what is left.

What the library validates away (HC_PHMM_EINVAL instead of the reference's
behaviour), so this file never meets it:
  * POS == 0 (get_alignment_begin() wraps to 2^32 - 1),
  * an empty CIGAR ("*": front() / back() of an empty vector),
  * an operator outside MIDNSHP=X,
  * a CIGAR whose read length differs from len(SEQ) (substr would throw
    std::out_of_range or clip bases that are not soft-clipped),
  * a negative window begin (the reference's size_t has none).
Reads the four flag filters remove are never inspected by either side.
"""
from __future__ import annotations

import re

U32 = (1 << 32) - 1
U64 = (1 << 64) - 1

MIN_MAPPING_QUALITY_SCORE = 20
MINIMUM_READ_LENGTH_AFTER_TRIMMING = 10

KEPT, MAPQ, DUPLICATE, SECONDARY, MATE_CONTIG, MIN_LENGTH = 0, 1, 2, 3, 4, 5


def parse_cigar(text: str):
    """Cigar::to_cigar_elements for well-formed text: a list of [length, op]."""
    return [[int(n), op] for n, op in re.findall(r"(\d+)(.)", text)]


def cigar_text(cigar) -> str:
    return "".join(f"{n}{op}" for n, op in cigar)


class SAMRecord:
    def __init__(self, FLAG, POS, MAPQ, CIGAR, RNEXT, SEQ, QUAL=None):
        self.FLAG, self.POS, self.MAPQ, self.RNEXT = FLAG, POS, MAPQ, RNEXT
        self.CIGAR = parse_cigar(CIGAR) if isinstance(CIGAR, str) else [list(e) for e in CIGAR]
        self.SEQ = SEQ
        self.QUAL = SEQ if QUAL is None else QUAL

    def READ_REVERSE_STRAND(self):
        return (self.FLAG & 0x10) != 0

    def SECONDARY_ALIGNMENT(self):
        return (self.FLAG & 0x100) != 0

    def DUPLICATE_READ(self):
        return (self.FLAG & 0x400) != 0

    def size(self):
        return len(self.SEQ)

    def get_alignment_begin(self):          # sam.hpp:69, uint32
        return (self.POS - 1) & U32

    def get_reference_length(self):         # cigar.hpp:92-111
        reference_length = 0
        for length, op in self.CIGAR:
            if op in ("M", "D", "N", "=", "X"):
                reference_length += length
        return reference_length

    def get_alignment_end(self):            # sam.hpp:71, size_t
        return (self.get_alignment_begin() + self.get_reference_length()) & U64

    def get_interval(self):                 # sam.hpp:72
        return self.get_alignment_begin(), self.get_alignment_end()


def substr(s: str, pos: int, n: int = U64) -> str:
    if pos > len(s):
        raise IndexError("basic_string::substr")
    return s[pos:pos + min(n, len(s) - pos)]


def revert_soft_clipped_bases(read: SAMRecord) -> None:     # read_clipper.hpp:32-66
    cigar = read.CIGAR
    if read.READ_REVERSE_STRAND():
        front_length, front_op = cigar[0]
        if front_op == "S":
            read.SEQ = substr(read.SEQ, front_length)
            read.QUAL = substr(read.QUAL, front_length)
        back_length, back_op = cigar[-1]
        if back_op == "S":
            cigar[-1] = [back_length, "M"]
    else:
        front_length, front_op = cigar[0]
        alignment_begin = read.get_alignment_begin()
        if front_op == "S" and alignment_begin >= front_length:
            cigar[0] = [front_length, "M"]
            read.POS = (alignment_begin - front_length + 1) & U32
        back_length, back_op = cigar[-1]
        if back_op == "S":
            read.SEQ = substr(read.SEQ, 0, (len(read.SEQ) - back_length) & U64)
            read.QUAL = substr(read.QUAL, 0, (len(read.QUAL) - back_length) & U64)


def hard_clip_to_interval(read: SAMRecord, begin: int, end: int) -> None:   # read_clipper.hpp:68-91
    alignment_begin = read.get_alignment_begin()
    alignment_end = read.get_alignment_end()
    if alignment_begin < begin:
        clip_size = (begin - alignment_begin) & U64
        if clip_size > len(read.SEQ):
            clip_size = len(read.SEQ)
        read.SEQ = substr(read.SEQ, clip_size)
        read.QUAL = substr(read.QUAL, clip_size)
    if alignment_end > end:
        clip_size = (alignment_end - end) & U64
        read.SEQ = substr(read.SEQ, 0, (len(read.SEQ) - clip_size) & U64)
        read.QUAL = substr(read.QUAL, 0, (len(read.QUAL) - clip_size) & U64)


FILTERS = ((MAPQ, lambda r: r.MAPQ < MIN_MAPPING_QUALITY_SCORE),       # haplotypecaller.hpp:52-66, in its order
           (DUPLICATE, lambda r: r.DUPLICATE_READ()),
           (SECONDARY, lambda r: r.SECONDARY_ALIGNMENT()),
           (MATE_CONTIG, lambda r: r.RNEXT != "="))


def prepare(reads, begin: int, end: int):
    """filter_reads + hard_clip_reads on a list of SAMRecord, in place as the
    reference does it (erase-remove keeps the order). Returns (survivors,
    reasons): the surviving records, and per input read the filter that removed
    it (KEPT for a survivor)."""
    reasons = [KEPT] * len(reads)
    alive = list(range(len(reads)))
    for code, pred in FILTERS:
        still = []
        for j in alive:
            if pred(reads[j]):
                reasons[j] = code
            else:
                still.append(j)
        alive = still
    for j in alive:
        revert_soft_clipped_bases(reads[j])
    for j in alive:
        hard_clip_to_interval(reads[j], begin, end)
    still = []
    for j in alive:
        if reads[j].size() < MINIMUM_READ_LENGTH_AFTER_TRIMMING:
            reasons[j] = MIN_LENGTH
        else:
            still.append(j)
    return [reads[j] for j in still], reasons


# ---- the library's record, derived from the restated strings ---------------------

def make_seq(n: int) -> str:
    """n distinct symbols, so that a surviving slice names its own offset."""
    return "".join(chr(0x100 + k) for k in range(n))


def records(window):
    """The hc_prep_record fields of every read of a window {begin, end, reads:
    [dict(flag, mapq, pos, cigar (text), mate_same, seq_len)]} and the window's
    totals, from the restatement run on make_seq() strings: offset and length
    are read off the surviving slice."""
    recs = []
    sam = []
    for r in window["reads"]:
        seq = make_seq(r["seq_len"])
        sam.append(SAMRecord(r["flag"], r["pos"], r["mapq"], r["cigar"], "=" if r["mate_same"] else "chrOther", seq))
    before = [(s.POS, [list(e) for e in s.CIGAR]) for s in sam]
    _, reasons = prepare(sam, window["begin"], window["end"])
    for r, s, reason, (pos0, cig0) in zip(window["reads"], sam, reasons, before):
        if reason in (MAPQ, DUPLICATE, SECONDARY, MATE_CONTIG):
            assert s.SEQ == make_seq(r["seq_len"]) and s.POS == pos0 and s.CIGAR == cig0   # never touched
            recs.append(dict(keep=0, drop_reason=reason, offset=0, length=r["seq_len"], new_pos=r["pos"],
                             front_to_M=0, back_to_M=0, begin=0, end=0))
            continue
        offset = (ord(s.SEQ[0]) - 0x100) if s.SEQ else None
        b, e = s.get_interval()
        front_to_M, back_to_M = int(s.CIGAR[0] != cig0[0]), int(s.CIGAR[-1] != cig0[-1])
        if len(cig0) == 1 and front_to_M:
            # one element is front() and back(): the reverse strand rewrites it as back(), the forward as front()
            front_to_M, back_to_M = (0, 1) if s.READ_REVERSE_STRAND() else (1, 0)
        recs.append(dict(keep=int(reason == KEPT), drop_reason=reason, offset=offset, length=len(s.SEQ), new_pos=s.POS,
                         front_to_M=front_to_M, back_to_M=back_to_M, begin=b, end=e))
    kept = [j for j, c in enumerate(recs) if c["keep"]]
    return dict(records=recs, kept=kept, n_kept=len(kept), kept_bases=sum(recs[j]["length"] for j in kept))


def same_record(got, exp) -> bool:
    """Field by field; the offset of an empty view is not defined by a string."""
    for k, v in exp.items():
        if k == "offset" and v is None:
            continue
        if got[k] != v:
            return False
    return True
