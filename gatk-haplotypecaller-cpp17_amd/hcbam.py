"""Python mirror of the MI355X BAM front (include/hc_bam.h).

``inflate(file)`` is one hc_bgzf_inflate: any BGZF file to dict(bytes,
compressed_offset, inflated_offset, isize), the last three per member.

``parse(bam)`` is one hc_bam_parse: dict(records, line_no, pool) as
hccontig.parse_sam gives them (``line`` is the record's offset in ``bases``,
line_no the record's 1-based ordinal), ref_id per record, ``header`` (the text),
``refs`` = [(name, length)] and ``bases``: per record SEQ as ASCII, then QUAL + 33.

``call_genome_bam(bam, contigs=[(name, ref), ...], ...)`` is one
hc_bam_genome_call: the dict of hcgenome.call_genome (read by hcgenome.results)
plus ``bases``, the buffer the records of ``sam`` point into.

No CPU path: raises BamError without the library or a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hcbind
import hccontig
import hcgenome
import hcphmm
from hcbind import i32p as _i32p, i64p as _i64p, u32p as _u32p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_bam.h")
DEFECT_QUAL_RANGE = 6
MAX_ISIZE = 65536


class BamError(hcgenome.GenomeError):
    prefix = "hc_bam"


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hcgenome.lib()
        vp = C.c_void_p
        vpp = C.POINTER(C.c_void_p)
        recpp = C.POINTER(C.POINTER(hccontig.Record))
        L.hc_bgzf_inflate.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp)]
        L.hc_bgzf_result_bytes.argtypes = [vp, vpp, _i64p]
        L.hc_bgzf_result_members.argtypes = [vp, C.POINTER(_i64p), C.POINTER(_i64p), C.POINTER(_i32p), _i32p]
        L.hc_bgzf_result_free.argtypes = [vp]
        L.hc_bam_parse.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp)]
        L.hc_bam_result_records.argtypes = [vp, recpp, C.POINTER(_i32p), _i32p, C.POINTER(_u32p), _i32p, C.POINTER(_i32p)]
        L.hc_bam_result_header.argtypes = [vp, vpp, _i64p, _i32p]
        L.hc_bam_result_reference.argtypes = [vp, C.c_int32, vpp, _i32p, _i64p]
        L.hc_bam_result_bases.argtypes = [vp, vpp, _i64p]
        L.hc_bam_result_free.argtypes = [vp]
        L.hc_bam_genome_call.argtypes = [C.c_char_p, C.c_int64, C.POINTER(hcgenome.Contig), C.c_int32, C.c_int32, C.c_int32,
                                         C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.hc_bam_genome_result_bases.argtypes = [vp, vpp, _i64p]
        _lib = L
    return _lib


def declared_symbols():
    """The entry points of hc_bam.h."""
    return hcbind.declared(HEADER, "hc_(?:bgzf|bam)_")


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, BamError)


def _bytes(accessor, h):
    p, n = C.c_void_p(), C.c_int64()
    _check(accessor(h, C.byref(p), C.byref(n)))
    return C.string_at(p, n.value) if n.value else b""


def inflate(file: bytes):
    L = lib()
    file = bytes(file)
    h = C.c_void_p()
    _check(L.hc_bgzf_inflate(file, len(file), C.byref(h)))
    try:
        co, io, sz, n = _i64p(), _i64p(), _i32p(), C.c_int32()
        _check(L.hc_bgzf_result_members(h, C.byref(co), C.byref(io), C.byref(sz), C.byref(n)))
        return dict(bytes=_bytes(L.hc_bgzf_result_bytes, h), compressed_offset=co[:n.value], inflated_offset=io[:n.value],
                    isize=sz[:n.value])
    finally:
        L.hc_bgzf_result_free(h)


def parse(bam: bytes):
    L = lib()
    bam = bytes(bam)
    h = C.c_void_p()
    _check(L.hc_bam_parse(bam, len(bam), C.byref(h)))
    try:
        rid = _i32p()

        def accessor(handle, *args):
            return L.hc_bam_result_records(handle, *args, C.byref(rid))
        out = hccontig._sam_arrays(h, accessor, False)
        n = len(out["line_no"])
        out["ref_id"] = np.array(rid[:n], np.int32) if n else np.zeros(0, np.int32)
        n_ref = C.c_int32()
        _check(L.hc_bam_result_header(h, None, None, C.byref(n_ref)))
        out["header"] = _bytes(lambda hh, p, m: L.hc_bam_result_header(hh, p, m, None), h)
        refs = []
        for k in range(n_ref.value):
            name, ln, length = C.c_void_p(), C.c_int32(), C.c_int64()
            _check(L.hc_bam_result_reference(h, k, C.byref(name), C.byref(ln), C.byref(length)))
            refs.append((C.string_at(name, ln.value).decode("latin-1"), length.value))
        out["refs"] = refs
        out["bases"] = _bytes(L.hc_bam_result_bases, h)
        return out
    finally:
        L.hc_bam_result_free(h)


class Prepared(hcgenome.Prepared):
    """The arguments of a call, built once (timing tools time run() alone); `sam` is the BAM file."""

    def run(self):
        """One hc_bam_genome_call; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_bam_genome_call(self.sam, len(self.sam), self.table, self.n, self.region_size, self.padding_size,
                                        self.seed & (2 ** 64 - 1), self.pick, self.flags, C.byref(h)))
        return h


def call_genome_bam(bam, contigs, region_size=245, padding_size=85, seed=0, pick="seeded", skip_unplaced=False,
                    use_double=None, want_site_reads=False, sorted_buckets=False, windows=None):
    p = Prepared(bam, contigs, region_size, padding_size, seed, pick, skip_unplaced, use_double, want_site_reads,
                 sorted_buckets)
    h = p.run()
    try:
        out = hcgenome.results(h, [n.decode("latin-1") for n in p.names], windows)
        out["bases"] = _bytes(lib().hc_bam_genome_result_bases, h)
        return out
    finally:
        p.free(h)
