"""A restatement in plain Python of the reference's top layer, HaplotypeCaller::
do_work (haplotypecaller.hpp:24-50, 112-154), for the tests of hc_sam.h and
hc_contig.h. It shares no code with the library.

    extract            operator>>(istream&, string&) on a Python string
    to_cigar_elements  cigar.hpp:57-68, with the syntax the library insists on
    parse_record       sam.hpp:100-114: the eleven extractions of one line
    load_all_reads     haplotypecaller.hpp:24-42: lines, header, records
    reads_map          :29-39: the per-position lists, with the placement rules
    window_bounds      :125-128, 148-151
    picks              :138-143 with the pick function injected
    pick_seeded        the library's own pick (include/hc_contig.h)
    vcf_header, variant_line, vcf   :132-135 and Variant::print

Where the reference reads uninitialised memory, indexes out of range or leaves
a stream in failbit, the issue defines an error or a skip instead; those rules
are restated here from their text in include/hc_sam.h and include/hc_contig.h.
Text is handled as str, one character per byte (latin-1).
"""
from __future__ import annotations

SPACE = " \t\n\v\f\r"          # the C locale's isspace
OPS = "MIDNSHP=X"
READ_OPS, MAX_CIGAR_LENGTH, MAX_READ_LEN = "MIS=X", (1 << 28) - 1, 65536
FIELDS = ("QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL")
MASK = (1 << 64) - 1


class SamSyntax(Exception):
    """A line the parser refuses: 1-based line number and "fields" or a field's name."""

    def __init__(self, line_no, field):
        super().__init__(f"line {line_no}: {field}")
        self.line_no, self.field = line_no, field


class Unplaced(Exception):
    def __init__(self, line_no):
        super().__init__(f"line {line_no}: unplaced")
        self.line_no = line_no


class Defective(Exception):
    def __init__(self, line_no, defect):
        super().__init__(f"line {line_no}: defect {defect}")
        self.line_no, self.defect = line_no, defect


def extract(s: str, i: int):
    """is >> token from position i: (token, start, next position); token None at the end of the stream."""
    while i < len(s) and s[i] in SPACE:
        i += 1
    if i == len(s):
        return None, i, i
    j = i
    while j < len(s) and s[j] not in SPACE:
        j += 1
    return s[i:j], i, j


def _number(tok: str, lo: int, hi: int):
    """Decimal digits, an optional '-' when lo < 0, value in [lo, hi]; None for anything else."""
    negative = lo < 0 and tok.startswith("-")
    body = tok[1:] if negative else tok
    if not body or any(c not in "0123456789" for c in body):
        return None
    v = -int(body) if negative else int(body)
    return v if lo <= v <= hi else None


def to_cigar_elements(s: str):
    """[(length, op)], [] for "*"; None for what is not a CIGAR."""
    if s == "*":
        return []
    out, i = [], 0
    while i < len(s):
        j = i
        while j < len(s) and s[j] in "0123456789":
            j += 1
        if j == i or j == len(s) or s[j] not in OPS:
            return None
        length = int(s[i:j])
        if length > MAX_CIGAR_LENGTH:
            return None
        out.append((length, s[j]))
        i = j + 1
    return out or None


def parse_record(line: str, line_no: int = 1):
    """One alignment line: None for a line without a token, a dict of the record's
    fields (offsets from the line's start, `elements` = the CIGAR) or SamSyntax."""
    toks, i = [], 0
    while len(toks) < 11:
        t, at, i = extract(line, i)
        if t is None:
            break
        toks.append((t, at))
    if not toks:
        return None
    if len(toks) < 11:
        raise SamSyntax(line_no, "fields")
    val = {}
    for name, k, lo, hi in (("FLAG", 1, 0, 65535), ("POS", 3, 0, 2 ** 32 - 1), ("MAPQ", 4, 0, 65535)):
        val[name] = _number(toks[k][0], lo, hi)
        if val[name] is None:
            raise SamSyntax(line_no, name)
    elements = to_cigar_elements(toks[5][0])
    if elements is None:
        raise SamSyntax(line_no, "CIGAR")
    if _number(toks[7][0], 0, 2 ** 32 - 1) is None:
        raise SamSyntax(line_no, "PNEXT")
    if _number(toks[8][0], -2 ** 31, 2 ** 31 - 1) is None:
        raise SamSyntax(line_no, "TLEN")
    seq, qual = toks[9], toks[10]
    read_length = sum(n for n, op in elements if op in READ_OPS)
    defect = (1 if val["POS"] == 0 else 2 if not elements else 3 if read_length != len(seq[0])
              else 4 if len(qual[0]) != len(seq[0]) else 5 if len(seq[0]) > MAX_READ_LEN else 0)
    return dict(seq_off=seq[1], qual_off=qual[1], seq_len=len(seq[0]), qual_len=len(qual[0]), pos=val["POS"],
                n_cigar=len(elements), flag=val["FLAG"], mapq=val["MAPQ"], mate_same_contig=int(toks[6][0] == "="),
                defect=defect, elements=elements, line_no=line_no)


def lines_of(text: str):
    """getline until it fails: [(offset, line)]; a text ending in '\\n' has no extra empty line."""
    out, at = [], 0
    while at < len(text):
        nl = text.find("\n", at)
        end = len(text) if nl < 0 else nl
        out.append((at, text[at:end]))
        at = end + 1
    return out


def load_all_reads(text):
    """dict(records, pool, n_header_lines): every alignment line's record in file
    order (`line` = the line's offset, `cigar` = its first word in the pool), the
    BAM-packed CIGAR words, and the length of the leading run of '@' lines.
    Raises the SamSyntax of the lowest offending line."""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("latin-1")
    lines = lines_of(text)
    header = 0
    while header < len(lines) and lines[header][1][:1] == "@":
        header += 1
    records, pool = [], []
    for k in range(header, len(lines)):
        at, line = lines[k]
        r = parse_record(line, k + 1)
        if r is None:
            continue
        r.update(line=at, cigar=len(pool))
        pool += [n << 4 | OPS.index(op) for n, op in r["elements"]]
        records.append(r)
    return dict(records=records, pool=pool, n_header_lines=header)


def passes_flag_filters(r):
    return r["mapq"] >= 20 and not r["flag"] & 0x400 and not r["flag"] & 0x100 and bool(r["mate_same_contig"])


def reads_map(records, ref_len: int, skip_unplaced: bool = False):
    """{alignment_begin: [record indices in file order]}. The lowest line that is
    unplaced (without skip_unplaced) or defective behind no flag filter raises."""
    out = {}
    for k, r in enumerate(records):
        placed = r["pos"] != 0 and r["pos"] - 1 < ref_len
        if not placed:
            if skip_unplaced:
                continue
            raise Unplaced(r["line_no"])
        if passes_flag_filters(r) and r["defect"]:
            raise Defective(r["line_no"], r["defect"])
        out.setdefault(r["pos"] - 1, []).append(k)
    return out


def window_bounds(ref_len: int, region: int = 245, padding: int = 85):
    """Per window (padded_begin, padded_end, origin_begin, origin_end), as the loop advances them."""
    n = (ref_len + region - 1) // region
    out = []
    origin = [0, region]
    padded = [0, region + padding]
    for _ in range(n):
        out.append((padded[0], padded[1], origin[0], origin[1]))
        origin = [origin[0] + region, origin[1] + region]
        padded = [origin[0] - padding, origin[1] + padding]
    return out


def picks(rmap, ref_len: int, region: int, padding: int, pick_fn):
    """Per window the picked record indices in ascending position; pick_fn(window, begin, count) -> index."""
    out = []
    for w, (pb, pe, _, _) in enumerate(window_bounds(ref_len, region, padding)):
        reads = []
        for begin in range(pb, pe):
            if begin < ref_len and rmap.get(begin):
                lst = rmap[begin]
                reads.append(lst[pick_fn(w, begin, len(lst))])
        out.append(reads)
    return out


def pick_seeded(seed: int, window: int, begin: int, count: int) -> int:
    z = (seed + 0x9E3779B97F4A7C15 * (window * 2 ** 32 + begin + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return ((z >> 32) * count) >> 32


def pick_first(window: int, begin: int, count: int) -> int:
    return 0


def pick_fn(pick: str, seed: int = 0):
    return pick_first if pick == "first" else (lambda w, b, c: pick_seeded(seed, w, b, c))


VCF_HEADER = ("##fileformat=VCFv4.2\n"
              "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n"
              "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA12878\n")


def variant_line(contig: str, begin: int, alleles, gt, gq: int) -> str:
    """Variant::print."""
    s = f"{contig}\t{begin + 1}\t.\t{alleles[0]}\t"
    for i in range(1, len(alleles)):
        s += alleles[i] + ("\t" if i == len(alleles) - 1 else ",")
    return s + f".\t.\t.\tGT:GQ\t{gt[0]}/{gt[1]}:{gq}\n"


def vcf(contig: str, sites) -> str:
    """The file do_work writes for these sites (dicts as hccall gives them), in their order."""
    out = VCF_HEADER
    for s in sites:
        if s["status"] == 0:
            alleles = [a.decode("latin-1") if isinstance(a, bytes) else a for a in s["alleles"]]
            out += variant_line(contig, s["begin"], alleles, (s["a1"], s["a2"]), s["genotype_quality"])
    return out
