"""Python mirror of the MI355X read preparation (include/hc_prep.h).

``prep_reads(windows)`` is one hc_prep_reads: filter_reads and hard_clip_reads
(reference haplotypecaller.hpp:93-94) for every window in one device pass. A
window is a dict {begin, end, reads}; a read is a dict {flag, mapq, pos, cigar,
mate_same, seq_len} whose cigar is SAM text or a sequence of packed words
(``pack_cigar``). Returns one dict per window: ``records`` (one dict per read
with the fields of hc_prep_record), ``kept`` (indices of the kept reads in
input order), ``n_kept`` and ``kept_bases``. No CPU path: raises PrepError
without the library or a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

import hcbind
import hcphmm
from hcbind import i32p as _i32p, i64p as _i64p, u32p as _u32p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_prep.h")
KEPT, DROP_MAPQ, DROP_DUPLICATE, DROP_SECONDARY, DROP_MATE_CONTIG, DROP_MIN_LENGTH = 0, 1, 2, 3, 4, 5
OPS = "MIDNSHP=X"


class PrepError(hcbind.Error):
    prefix = "hc_prep"


class Read(C.Structure):
    _fields_ = [("cigar", _u32p), ("n_cigar", C.c_int32), ("pos", C.c_uint32), ("seq_len", C.c_int32),
                ("flag", C.c_uint16), ("mapq", C.c_uint16), ("mate_same_contig", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class Window(C.Structure):
    _fields_ = [("padded_begin", C.c_int64), ("padded_end", C.c_int64), ("reads", C.POINTER(Read)),
                ("n_reads", C.c_int32)]


class Record(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("new_pos", C.c_uint32), ("offset", C.c_int32),
                ("length", C.c_int32), ("keep", C.c_uint8), ("drop_reason", C.c_uint8), ("front_to_M", C.c_uint8),
                ("back_to_M", C.c_uint8)]


RECORD_DTYPE = np.dtype([("begin", "<i8"), ("end", "<i8"), ("new_pos", "<u4"), ("offset", "<i4"), ("length", "<i4"),
                         ("keep", "u1"), ("drop_reason", "u1"), ("front_to_M", "u1"), ("back_to_M", "u1")])

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hcphmm.lib()
        hcphmm.check_build_id()   # a stale binary would not have these entry points
        vp = C.c_void_p
        L.hc_prep_reads.argtypes = [C.POINTER(Window), C.c_int32, C.POINTER(vp)]
        L.hc_prep_result_window.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(Record)), _i32p, C.POINTER(_i32p), _i32p,
                                            _i64p]
        L.hc_prep_result_free.argtypes = [vp]
        _lib = L
    return _lib


def declared_symbols(header: str = HEADER):
    return hcbind.declared(header, "hc_prep_")


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, PrepError)


def pack_cigar(text: str):
    """SAM CIGAR text -> BAM-packed words (length << 4 | op); "*" is no word."""
    if text in ("", "*"):
        return np.zeros(0, np.uint32)
    parts = re.findall(r"(\d+)([A-Za-z=])", text)
    if "".join(n + op for n, op in parts) != text:
        raise ValueError(f"not a CIGAR: {text!r}")
    words = []
    for n, op in parts:
        if op not in OPS or int(n) >= 1 << 28:
            raise ValueError(f"not a CIGAR: {text!r}")
        words.append(int(n) << 4 | OPS.index(op))
    return np.array(words, np.uint32)


def read_structs(reads, keep_alive):
    """The hc_prep_read array of a window's read dicts (also hccall's)."""
    ra = (Read * max(len(reads), 1))()
    for j, r in enumerate(reads):
        cig = r["cigar"]
        words = pack_cigar(cig) if isinstance(cig, str) else np.ascontiguousarray(cig, np.uint32)
        keep_alive.append(words)
        ra[j] = Read(words.ctypes.data_as(_u32p) if len(words) else None, len(words), int(r["pos"]), int(r["seq_len"]),
                     int(r["flag"]), int(r["mapq"]), 1 if r["mate_same"] else 0)
    keep_alive.append(ra)
    return ra


class Prepared:
    """The C structs of a call, built once (timing tools time run() alone)."""

    def __init__(self, windows):
        self.n = len(windows)
        self.arr = (Window * max(self.n, 1))()
        self.keep_alive = []
        for k, w in enumerate(windows):
            ra = read_structs(w["reads"], self.keep_alive)
            self.arr[k] = Window(int(w["begin"]), int(w["end"]), ra if len(w["reads"]) else None, len(w["reads"]))

    def run(self):
        """One hc_prep_reads; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_prep_reads(self.arr, self.n, C.byref(h)))
        return h

    @staticmethod
    def free(h):
        lib().hc_prep_result_free(h)


def window_arrays(h, window: int, accessor=None):
    """(records as a RECORD_DTYPE array, kept indices, n_kept, kept_bases) of one window."""
    rec, kept = C.POINTER(Record)(), _i32p()
    nr, nk, kb = C.c_int32(), C.c_int32(), C.c_int64()
    _check((accessor or lib().hc_prep_result_window)(h, window, C.byref(rec), C.byref(nr), C.byref(kept), C.byref(nk),
                                                     C.byref(kb)))
    if nr.value:
        raw = C.string_at(rec, nr.value * C.sizeof(Record))
        recs = np.frombuffer(raw, RECORD_DTYPE).copy()
    else:
        recs = np.zeros(0, RECORD_DTYPE)
    k = np.array(kept[:nk.value], np.int32) if nk.value else np.zeros(0, np.int32)
    return recs, k, nk.value, kb.value


def window_dict(h, window: int, accessor=None):
    recs, kept, nk, kb = window_arrays(h, window, accessor)
    return dict(records=[{f: int(r[f]) for f in RECORD_DTYPE.names} for r in recs], kept=[int(x) for x in kept],
                n_kept=nk, kept_bases=kb)


def prep_reads(windows):
    p = Prepared(windows)
    h = p.run()
    try:
        return [window_dict(h, w) for w in range(p.n)]
    finally:
        p.free(h)
