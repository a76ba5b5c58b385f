"""Python mirror of the MI355X SAM parser (include/hc_sam.h) and contig caller
(include/hc_contig.h).

``parse_sam(text)`` is one hc_sam_parse: the bytes of a SAM file to a dict
``records`` (a RECORD_DTYPE array, one per alignment line), ``line_no`` (each
record's 1-based line), ``pool`` (BAM-packed CIGAR words; record k's are
pool[cigar : cigar + n_cigar]) and ``n_header_lines``. SEQ and QUAL are views:
``seq(text, rec)`` and ``qual(text, rec)`` slice them out of the text.

``call_contig(sam, contig, ref, ...)`` is one hc_contig_call:
HaplotypeCaller::do_work (reference haplotypecaller.hpp:112-154) from the SAM
text and the contig's (upper-cased) reference to the VCF text. Returns a dict:
``vcf`` (bytes), ``windows`` (per window: padded_begin, padded_end,
origin_begin, origin_end, ref_len, picked = record indices, status, asm_status,
kmer_size, n_haps, reads = the surviving record indices), ``sites`` (records as
hccall.call_windows gives them, ``region`` = the window's index) and ``sam`` as
parse_sam gives it. No CPU path: raises ContigError without the library or a
gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hcbind
import hccall
import hcgt
import hcphmm
import hcregion
from hcbind import i32p as _i32p, i64p as _i64p, u32p as _u32p

HEADER_SAM = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_sam.h")
HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_contig.h")
DEFECT_NONE, DEFECT_POS_ZERO, DEFECT_NO_CIGAR, DEFECT_CIGAR_LENGTH, DEFECT_QUAL_LENGTH, DEFECT_TOO_LONG = range(6)
F64, DEFAULT_MODE, WANT_SITE_READS, SKIP_UNPLACED = 1, 2, 32, 256   # the first three are hcregion's bits
PICK_SEEDED, PICK_FIRST = 0, 1
PICKS = dict(seeded=PICK_SEEDED, first=PICK_FIRST)


class ContigError(hcbind.Error):
    prefix = "hc_contig"


class Record(C.Structure):
    _fields_ = [("line", C.c_int64), ("seq_off", C.c_uint32), ("qual_off", C.c_uint32), ("seq_len", C.c_int32),
                ("qual_len", C.c_int32), ("pos", C.c_uint32), ("cigar", C.c_int32), ("n_cigar", C.c_int32),
                ("flag", C.c_uint16), ("mapq", C.c_uint16), ("mate_same_contig", C.c_uint8), ("defect", C.c_uint8),
                ("reserved", C.c_uint8 * 6)]


RECORD_DTYPE = np.dtype([("line", "<i8"), ("seq_off", "<u4"), ("qual_off", "<u4"), ("seq_len", "<i4"),
                         ("qual_len", "<i4"), ("pos", "<u4"), ("cigar", "<i4"), ("n_cigar", "<i4"), ("flag", "<u2"),
                         ("mapq", "<u2"), ("mate_same_contig", "u1"), ("defect", "u1"), ("reserved", "u1", (6,))])

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hccall.lib()
        hcphmm.check_build_id()   # a stale binary would not have these entry points
        vp = C.c_void_p
        recpp = C.POINTER(C.POINTER(Record))
        L.hc_sam_parse.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp)]
        L.hc_sam_result_records.argtypes = [vp, recpp, C.POINTER(_i32p), _i32p, C.POINTER(_u32p), _i32p, _i32p]
        L.hc_sam_result_free.argtypes = [vp]
        L.hc_contig_call.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.hc_contig_result_vcf.argtypes = [vp, C.POINTER(C.c_void_p), _i64p, _i32p]
        L.hc_contig_result_sam.argtypes = [vp, recpp, C.POINTER(_i32p), _i32p, C.POINTER(_u32p), _i32p]
        L.hc_contig_result_window.argtypes = [vp, C.c_int32, _i64p, _i64p, _i64p, _i64p, _i32p, C.POINTER(_i32p), _i32p,
                                              _i32p, _i32p, _i32p, _i32p]
        L.hc_contig_result_sites.argtypes = [vp, C.POINTER(C.POINTER(hcgt.CallSite)), _i64p]
        L.hc_contig_result_reads.argtypes = [vp, C.c_int32, C.POINTER(_i32p), _i32p]
        L.hc_contig_result_free.argtypes = [vp]
        _lib = L
    return _lib


def declared_symbols(header: str | None = None):
    """The entry points of hc_sam.h and hc_contig.h (or of `header` alone)."""
    return sorted(s for h in ([header] if header else [HEADER_SAM, HEADER]) for s in hcbind.declared(h, "hc_(?:sam|contig)_"))


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, ContigError)


def _sam_arrays(h, accessor, with_header):
    rec, ln, pool = C.POINTER(Record)(), _i32p(), _u32p()
    n, nw, nh = C.c_int32(), C.c_int32(), C.c_int32()
    args = [h, C.byref(rec), C.byref(ln), C.byref(n), C.byref(pool), C.byref(nw)]
    _check(accessor(*(args + ([C.byref(nh)] if with_header else []))))
    records = (np.frombuffer(C.string_at(rec, n.value * C.sizeof(Record)), RECORD_DTYPE).copy() if n.value
               else np.zeros(0, RECORD_DTYPE))
    line_no = np.array(ln[:n.value], np.int32) if n.value else np.zeros(0, np.int32)
    words = (np.frombuffer(C.string_at(pool, nw.value * 4), np.uint32).copy() if nw.value else np.zeros(0, np.uint32))
    out = dict(records=records, line_no=line_no, pool=words)
    if with_header:
        out["n_header_lines"] = nh.value
    return out


def parse_sam(text: bytes):
    L = lib()
    text = bytes(text)
    h = C.c_void_p()
    _check(L.hc_sam_parse(text, len(text), C.byref(h)))
    try:
        return _sam_arrays(h, L.hc_sam_result_records, True)
    finally:
        L.hc_sam_result_free(h)


def seq(text: bytes, rec) -> bytes:
    at = int(rec["line"]) + int(rec["seq_off"])
    return text[at:at + int(rec["seq_len"])]


def qual(text: bytes, rec) -> bytes:
    at = int(rec["line"]) + int(rec["qual_off"])
    return text[at:at + int(rec["qual_len"])]


class Prepared:
    """The arguments of a call, built once (timing tools time run() alone)."""

    def __init__(self, sam, contig, ref, region_size=245, padding_size=85, seed=0, pick="seeded", skip_unplaced=False,
                 use_double=None, want_site_reads=False):
        self.sam, self.ref = bytes(sam), bytes(ref)
        self.contig = contig.encode() if isinstance(contig, str) else bytes(contig)
        self.region_size, self.padding_size, self.seed, self.pick = region_size, padding_size, seed, PICKS[pick]
        self.flags = (hcregion.flags_of(want_site_reads=want_site_reads, use_double=use_double)
                      | (SKIP_UNPLACED if skip_unplaced else 0))

    def run(self):
        """One hc_contig_call; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_contig_call(self.sam, len(self.sam), self.contig, self.ref, len(self.ref), self.region_size,
                                    self.padding_size, self.seed & (2 ** 64 - 1), self.pick, self.flags, C.byref(h)))
        return h

    @staticmethod
    def free(h):
        lib().hc_contig_result_free(h)


def _sites(h):
    """The site records, as hccall.call_windows gives them."""
    return hcbind.call_sites(h, lib().hc_contig_result_sites, _check)


def results(h):
    L = lib()
    text, length, nw = C.c_void_p(), C.c_int64(), C.c_int32()
    _check(L.hc_contig_result_vcf(h, C.byref(text), C.byref(length), C.byref(nw)))
    wins = []
    for w in range(nw.value):
        b = [C.c_int64() for _ in range(4)]
        rl, npk, st, ast, k, nh = (C.c_int32() for _ in range(6))
        pk = _i32p()
        _check(L.hc_contig_result_window(h, w, *[C.byref(x) for x in b], C.byref(rl), C.byref(pk), C.byref(npk),
                                         C.byref(st), C.byref(ast), C.byref(k), C.byref(nh)))
        p, m = _i32p(), C.c_int32()
        _check(L.hc_contig_result_reads(h, w, C.byref(p), C.byref(m)))
        wins.append(dict(padded_begin=b[0].value, padded_end=b[1].value, origin_begin=b[2].value, origin_end=b[3].value,
                         ref_len=rl.value, picked=[int(pk[i]) for i in range(npk.value)], status=st.value,
                         asm_status=ast.value, kmer_size=k.value, n_haps=nh.value,
                         reads=[int(p[i]) for i in range(m.value)]))
    return dict(vcf=C.string_at(text, length.value), windows=wins, sites=_sites(h),
                sam=_sam_arrays(h, L.hc_contig_result_sam, False))


def call_contig(sam, contig, ref, region_size=245, padding_size=85, seed=0, pick="seeded", skip_unplaced=False,
                use_double=None, want_site_reads=False):
    p = Prepared(sam, contig, ref, region_size, padding_size, seed, pick, skip_unplaced, use_double, want_site_reads)
    h = p.run()
    try:
        return results(h)
    finally:
        p.free(h)
