"""A restatement in plain Python of the genome caller's rules (include/hc_genome.h),
on top of sam_restate.py: the RNAME of every record, the placement against a
contig table, per contig the windows and picks of do_work with genome-wide
window numbers, the FASTA reader applied until the file ends, and the VCF over
several contigs. It shares no code with the library.

    rnames            per record the third token of its line
    contig_of         per record the table index of its RNAME, or -1
    place             the per-contig, per-position lists with the placement rules
    genome_windows    every contig's windows and picks, in table order
    filtered          the stand-in text of one contig: header + the lines of its RNAME
    read_fasta        fasta.hpp:23-46 until the file ends
    vcf               the header once, then every contig's lines

The stand-in rule is the oracle of the tests: contig c's part of a genome call
equals a contig call (sam_restate on the CPU, hc_contig_call on the GPU) on
filtered(text, name of c), record indices translated by the map filtered()
returns.
"""
from __future__ import annotations

import functools

import sam_restate as SR

MAX_READS_PER_POSITION = 4096


class TooDeep(Exception):
    def __init__(self, contig, position):
        super().__init__(f"contig {contig}: more than {MAX_READS_PER_POSITION} reads at position {position}")
        self.contig, self.position = contig, position


def _text(text):
    return bytes(text).decode("latin-1") if isinstance(text, (bytes, bytearray)) else text


@functools.lru_cache(maxsize=4)
def _parsed(sam: bytes):
    return SR.load_all_reads(sam)


def rnames(text, records):
    """Per record of load_all_reads(text) its RNAME."""
    text = _text(text)
    out = []
    for r in records:
        i = r["line"]
        for _ in range(3):
            tok, _, i = SR.extract(text, i)
        out.append(tok)
    return out


def contig_of(text, records, names):
    index = {}
    for k, n in enumerate(names):
        assert n not in index and n and n != "*" and len(n) <= 255
        index[n] = k
    return [index.get(n, -1) for n in rnames(text, records)]


def place(records, of, ref_lens, skip_unplaced=False):
    """Per contig {alignment_begin: [record indices in file order]}. The lowest
    line that is unplaced (without skip_unplaced) or defective behind no flag
    filter raises; then the lowest (contig, position) that is too deep."""
    maps = [dict() for _ in ref_lens]
    for k, r in enumerate(records):
        c = of[k]
        if c < 0 or r["pos"] == 0 or r["pos"] - 1 >= ref_lens[c]:
            if skip_unplaced:
                continue
            raise SR.Unplaced(r["line_no"])
        if SR.passes_flag_filters(r) and r["defect"]:
            raise SR.Defective(r["line_no"], r["defect"])
        maps[c].setdefault(r["pos"] - 1, []).append(k)
    for c, m in enumerate(maps):
        for begin in sorted(m):
            if len(m[begin]) > MAX_READS_PER_POSITION:
                raise TooDeep(c, begin + 1)
    return maps


def genome_windows(sam, contigs, pick="seeded", seed=0, skip_unplaced=False, region=245, padding=85):
    """contigs = [(name, ref)]. Returns dict(parsed, contig_of, contigs = per contig
    first_window / n_windows / n_records, windows = per genome-wide window its
    contig, bounds inside the contig, ref_len and picked record indices)."""
    parsed = SR.load_all_reads(sam)
    recs = parsed["records"]
    names = [n for n, _ in contigs]
    of = contig_of(sam, recs, names)
    maps = place(recs, of, [len(r) for _, r in contigs], skip_unplaced)
    fn = SR.pick_fn(pick, seed)
    wins, per = [], []
    for c, (name, ref) in enumerate(contigs):
        bounds = SR.window_bounds(len(ref), region, padding)
        picked = SR.picks(maps[c], len(ref), region, padding, fn)   # the contig's own window index and positions
        per.append(dict(name=name, first_window=len(wins), n_windows=len(bounds), n_records=of.count(c)))
        for (pb, pe, ob, oe), idx in zip(bounds, picked):
            wins.append(dict(contig=c, padded_begin=pb, padded_end=pe, origin_begin=ob, origin_end=oe,
                             ref_len=len(ref[pb:pe]), picked=idx))
    return dict(parsed=parsed, contig_of=of, contigs=per, windows=wins)


@functools.lru_cache(maxsize=64)
def filtered(sam: bytes, name: str):
    """(the header lines + the alignment lines whose RNAME is `name`, in file
    order, as bytes; per record of that text its index among the whole text's records)."""
    text = _text(sam)
    parsed = _parsed(sam)
    lines = SR.lines_of(text)
    at = {off: k for k, (off, _) in enumerate(lines)}
    keep = [ln + "\n" for _, ln in lines[:parsed["n_header_lines"]]]
    index = []
    for k, (r, n) in enumerate(zip(parsed["records"], rnames(text, parsed["records"]))):
        if n == name:
            keep.append(lines[at[r["line"]]][1] + "\n")
            index.append(k)
    return "".join(keep).encode("latin-1"), index


def read_fasta(text):
    """[(name, upper-cased sequence)]: operator>> applied until the stream ends.
    ValueError where the reference would swallow a header into the sequence (a
    header line directly followed by a header line or by the end)."""
    text = _text(text)
    lines = [ln for _, ln in SR.lines_of(text)]
    out, k = [], 0
    while k < len(lines):
        if lines[k][:1] != ">":
            raise ValueError("expected '>'")
        header = lines[k][1:]
        stop = [i for i, ch in enumerate(header) if ch in " \t\v\f\r"]
        name = header[:stop[0]] if stop else header
        k += 1
        if k == len(lines) or lines[k][:1] == ">":
            raise ValueError("a header without a sequence line")
        seq = ""
        while k < len(lines):
            seq += lines[k]          # appended as it is
            k += 1
            if k < len(lines) and lines[k][:1] == ">":   # is.peek() == '>'
                break
        out.append((name, seq.upper()))
    return out


def vcf(names, windows, sites) -> str:
    """The header once, then the sites in their order (genome-wide window order
    is table order); CHROM is the name of the site's window's contig."""
    out = SR.VCF_HEADER
    for s in sites:
        out += SR.vcf(names[windows[s["region"]]["contig"]], [s])[len(SR.VCF_HEADER):]
    return out
