"""Python mirror of the MI355X genome caller (include/hc_genome.h).

``call_genome(sam, contigs=[(name, ref), ...], ...)`` is one hc_genome_call:
the text of a SAM file with reads of many contigs and the contigs' (upper-cased)
references to one VCF text. Returns the dict of hccontig.call_contig with
windows numbered genome-wide, plus ``contigs`` (per contig of the table: name,
first_window, n_windows, n_records = the records whose RNAME is its name),
``contig`` in each window (bounds are positions inside that contig) and
``contig_of`` in ``sam`` (per record the table index of its RNAME, or -1).
Every contig's picks use the same seed.

``sorted_buckets=True`` sets HC_GENOME_SORTED_BUCKETS: the buckets come from a
sort sized by the records, not from arrays over every base of the table; the
result is the same in every field. ``HC_GENOME_BUCKETS=sorted`` in the
environment does the same for a caller that cannot pass the argument.
``windows=`` (an iterable of genome-wide window indices) makes ``results`` and
``call_genome`` read back those windows only, in that order, where a table has
millions of them; the default is every window.

``read_fasta(text)`` reads every record of a FASTA text as the reference's
operator>> (fasta/fasta.hpp:23-46) reads one: [(name, upper-cased sequence)].

No CPU path: raises GenomeError without the library or a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hcbind
import hccontig
import hcgt
import hcphmm
import hcregion
from hcbind import i32p as _i32p, i64p as _i64p, u32p as _u32p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_genome.h")
MAX_NAME_LEN = 255
PICKS = hccontig.PICKS
SKIP_UNPLACED = hccontig.SKIP_UNPLACED
SORTED_BUCKETS = 512


class GenomeError(hcbind.Error):
    prefix = "hc_genome"


class Contig(C.Structure):
    """hc_genome_contig."""
    _fields_ = [("name", C.c_char_p), ("ref", C.c_char_p), ("ref_len", C.c_int64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hccontig.lib()
        vp = C.c_void_p
        recpp = C.POINTER(C.POINTER(hccontig.Record))
        L.hc_genome_call.argtypes = [C.c_char_p, C.c_int64, C.POINTER(Contig), C.c_int32, C.c_int32, C.c_int32, C.c_uint64,
                                     C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.hc_genome_result_vcf.argtypes = [vp, C.POINTER(C.c_void_p), _i64p, _i32p, _i32p]
        L.hc_genome_result_contig.argtypes = [vp, C.c_int32, _i32p, _i32p, _i32p]
        L.hc_genome_result_sam.argtypes = [vp, recpp, C.POINTER(_i32p), _i32p, C.POINTER(_u32p), _i32p, C.POINTER(_i32p)]
        L.hc_genome_result_window.argtypes = [vp, C.c_int32, _i32p, _i64p, _i64p, _i64p, _i64p, _i32p, C.POINTER(_i32p),
                                              _i32p, _i32p, _i32p, _i32p, _i32p]
        L.hc_genome_result_sites.argtypes = [vp, C.POINTER(C.POINTER(hcgt.CallSite)), _i64p]
        L.hc_genome_result_reads.argtypes = [vp, C.c_int32, C.POINTER(_i32p), _i32p]
        L.hc_genome_result_free.argtypes = [vp]
        _lib = L
    return _lib


def declared_symbols():
    """The entry points of hc_genome.h."""
    return hcbind.declared(HEADER, "hc_genome_")


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, GenomeError)


def read_fasta(text):
    """[(name, upper-cased sequence)] of every record. The name runs to the first
    of " \\t\\v\\f\\r", the lines are appended as they are. ValueError for a text
    that does not begin with '>' and for a header line directly followed by
    another header line or by the end of the text (the reference would take the
    second header for sequence)."""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("latin-1")
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()             # getline fails after the last newline
    out, k = [], 0
    while k < len(lines):
        if not lines[k].startswith(">"):
            raise ValueError("error: expected '>'")
        header = lines[k][1:]
        cut = min([header.find(c) for c in " \t\v\f\r" if c in header] or [len(header)])
        k += 1
        if k == len(lines) or lines[k].startswith(">"):
            raise ValueError(f"FASTA record {header[:cut]!r} has no sequence line")
        seq = []
        while k < len(lines) and not lines[k].startswith(">"):
            seq.append(lines[k])
            k += 1
        out.append((header[:cut], "".join(seq).upper()))
    return out


class Prepared:
    """The arguments of a call, built once (timing tools time run() alone)."""

    def __init__(self, sam, contigs, region_size=245, padding_size=85, seed=0, pick="seeded", skip_unplaced=False,
                 use_double=None, want_site_reads=False, sorted_buckets=False):
        self.sam = bytes(sam)
        self.names = [n.encode("latin-1") if isinstance(n, str) else bytes(n) for n, _ in contigs]
        self.refs = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for _, r in contigs]
        self.table = (Contig * max(len(contigs), 1))()
        for k, (n, r) in enumerate(zip(self.names, self.refs)):
            self.table[k] = Contig(n, r, len(r))
        self.n = len(contigs)
        self.region_size, self.padding_size, self.seed, self.pick = region_size, padding_size, seed, PICKS[pick]
        self.flags = (hcregion.flags_of(want_site_reads=want_site_reads, use_double=use_double)
                      | (SKIP_UNPLACED if skip_unplaced else 0) | (SORTED_BUCKETS if sorted_buckets else 0))

    def run(self):
        """One hc_genome_call; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_genome_call(self.sam, len(self.sam), self.table, self.n, self.region_size, self.padding_size,
                                    self.seed & (2 ** 64 - 1), self.pick, self.flags, C.byref(h)))
        return h

    @staticmethod
    def free(h):
        lib().hc_genome_result_free(h)


def results(h, names, windows=None):
    L = lib()
    text, length, nw, nc = C.c_void_p(), C.c_int64(), C.c_int32(), C.c_int32()
    _check(L.hc_genome_result_vcf(h, C.byref(text), C.byref(length), C.byref(nw), C.byref(nc)))
    contigs = []
    for c in range(nc.value):
        fw, n, nr = C.c_int32(), C.c_int32(), C.c_int32()
        _check(L.hc_genome_result_contig(h, c, C.byref(fw), C.byref(n), C.byref(nr)))
        contigs.append(dict(name=names[c], first_window=fw.value, n_windows=n.value, n_records=nr.value))
    wins = []
    for w in (range(nw.value) if windows is None else windows):
        b = [C.c_int64() for _ in range(4)]
        ct, rl, npk, st, ast, k, nh = (C.c_int32() for _ in range(7))
        pk = _i32p()
        _check(L.hc_genome_result_window(h, w, C.byref(ct), *[C.byref(x) for x in b], C.byref(rl), C.byref(pk),
                                         C.byref(npk), C.byref(st), C.byref(ast), C.byref(k), C.byref(nh)))
        p, m = _i32p(), C.c_int32()
        _check(L.hc_genome_result_reads(h, w, C.byref(p), C.byref(m)))
        wins.append(dict(contig=ct.value, padded_begin=b[0].value, padded_end=b[1].value, origin_begin=b[2].value,
                         origin_end=b[3].value, ref_len=rl.value, picked=pk[:npk.value], status=st.value,
                         asm_status=ast.value, kmer_size=k.value, n_haps=nh.value, reads=p[:m.value]))
    of = _i32p()

    def sam_accessor(handle, *args):
        return L.hc_genome_result_sam(handle, *args, C.byref(of))
    sam = hccontig._sam_arrays(h, sam_accessor, False)
    n = len(sam["line_no"])
    sam["contig_of"] = np.array(of[:n], np.int32) if n else np.zeros(0, np.int32)
    return dict(vcf=C.string_at(text, length.value), contigs=contigs, windows=wins,
                sites=hcbind.call_sites(h, L.hc_genome_result_sites, _check), sam=sam)


def call_genome(sam, contigs, region_size=245, padding_size=85, seed=0, pick="seeded", skip_unplaced=False,
                use_double=None, want_site_reads=False, sorted_buckets=False, windows=None):
    p = Prepared(sam, contigs, region_size, padding_size, seed, pick, skip_unplaced, use_double, want_site_reads,
                 sorted_buckets)
    h = p.run()
    try:
        return results(h, [n.decode("latin-1") for n in p.names], windows)
    finally:
        p.free(h)
