"""Python mirror of the MI355X window caller (include/hc_call.h).

``call_windows(windows)`` is one hc_call_windows: HaplotypeCaller::call_region
(reference haplotypecaller.hpp:83-107) for every window, from aligned reads to
variants. A window is a dict {ref, padded_begin, padded_end, origin_begin,
origin_end, reads}; a read is hcprep's dict plus ``bases`` and ``quals``
(bytes of seq_len). Returns a dict: ``windows`` (per window: status,
asm_status, kmer_size, haps [(bases, score)], ``prep`` as hcprep gives it,
``reads`` = the indices of the reads that survive both filters, and on request
``L`` and ``alignments`` [(begin, cigar)]) and ``sites`` (records as
hcregion.call_regions gives them, ``region`` = the window's index). No CPU
path: raises CallError without the library or a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hcbind
import hcgt
import hcphmm
import hcprep
import hcregion
from hcbind import f64p as _f64p, i32p as _i32p, i64p as _i64p, u8p as _u8p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_call.h")
CALLED, NO_READS, NO_VARIATION = 0, 1, 2


class CallError(hcbind.Error):
    prefix = "hc_call"


class Window(C.Structure):
    _fields_ = [("ref", C.c_char_p), ("ref_len", C.c_int32), ("padded_begin", C.c_int64), ("padded_end", C.c_int64),
                ("origin_begin", C.c_int64), ("origin_end", C.c_int64), ("reads", C.POINTER(hcprep.Read)),
                ("bases", C.POINTER(C.c_char_p)), ("quals", C.POINTER(C.c_char_p)), ("n_reads", C.c_int32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        hcprep.lib()
        hcregion.lib()
        L = hcgt.lib()
        vp = C.c_void_p
        L.hc_call_windows.argtypes = [C.POINTER(Window), C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.hc_call_result_window.argtypes = [vp, C.c_int32, _i32p, _i32p, _i32p, _i32p]
        L.hc_call_result_prep.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(hcprep.Record)), _i32p, C.POINTER(_i32p),
                                          _i32p, _i64p]
        L.hc_call_result_hap.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(_u8p), _i32p, _f64p, _i32p,
                                         C.POINTER(C.c_char_p)]
        L.hc_call_result_sites.argtypes = [vp, C.POINTER(C.POINTER(hcgt.CallSite)), _i64p]
        L.hc_call_result_reads.argtypes = [vp, C.c_int32, C.POINTER(_i32p), _i32p]
        L.hc_call_result_matrix.argtypes = [vp, C.c_int32, C.POINTER(_f64p), _i32p, _i32p]
        L.hc_call_result_free.argtypes = [vp]
        _lib = L
    return _lib


def declared_symbols(header: str = HEADER):
    return hcbind.declared(header, "hc_call_")


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, CallError)


flags_of = hcregion.flags_of   # the HC_CALL_* bits are the HC_REGION_* bits


class Prepared:
    """The C structs of a call, built once (timing tools time run() alone)."""

    def __init__(self, windows):
        self.n = len(windows)
        self.arr = (Window * max(self.n, 1))()
        self.keep_alive = []
        for k, w in enumerate(windows):
            reads = w["reads"]
            ra = hcprep.read_structs(reads, self.keep_alive)
            ba = (C.c_char_p * max(len(reads), 1))(*[r["bases"] for r in reads])
            qa = (C.c_char_p * max(len(reads), 1))(*[r["quals"] for r in reads])
            for j, r in enumerate(reads):
                if len(r["bases"]) != r["seq_len"] or len(r["quals"]) != r["seq_len"]:
                    raise CallError(hcphmm.EINVAL, f"window {k} read {j}: bases / quals are not seq_len long")
            self.keep_alive += [ba, qa]
            ref = w["ref"]
            nr = len(reads)
            self.arr[k] = Window(ref, 0 if ref is None else len(ref), int(w["padded_begin"]), int(w["padded_end"]),
                                 int(w["origin_begin"]), int(w["origin_end"]), ra if nr else None,
                                 ba if nr else None, qa if nr else None, nr)

    def run(self, flags: int):
        """One hc_call_windows; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_call_windows(self.arr, self.n, flags, C.byref(h)))
        return h

    @staticmethod
    def free(h):
        lib().hc_call_result_free(h)


def _sites(h):
    return hcbind.call_sites(h, lib().hc_call_result_sites, _check)


def results(h, n, want_L=False, want_cigars=False):
    L = lib()
    wins = []
    for w in range(n):
        status, ast, k, nh = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(L.hc_call_result_window(h, w, C.byref(status), C.byref(ast), C.byref(k), C.byref(nh)))
        rec = dict(status=status.value, asm_status=ast.value, kmer_size=k.value, haps=[],
                   prep=hcprep.window_dict(h, w, L.hc_call_result_prep))
        if want_cigars:
            rec["alignments"] = []
        for j in range(nh.value):
            b, ln, sc = _u8p(), C.c_int32(), C.c_double()
            if want_cigars:
                beg, cig = C.c_int32(), C.c_char_p()
                _check(L.hc_call_result_hap(h, w, j, C.byref(b), C.byref(ln), C.byref(sc), C.byref(beg), C.byref(cig)))
                rec["alignments"].append((beg.value, None if cig.value is None else cig.value.decode()))
            else:
                _check(L.hc_call_result_hap(h, w, j, C.byref(b), C.byref(ln), C.byref(sc), None, None))
            rec["haps"].append((C.string_at(b, ln.value), sc.value))
        p, m = _i32p(), C.c_int32()
        _check(L.hc_call_result_reads(h, w, C.byref(p), C.byref(m)))
        rec["reads"] = [int(p[i]) for i in range(m.value)]
        if want_L:
            lp, nr, nhh = _f64p(), C.c_int32(), C.c_int32()
            _check(L.hc_call_result_matrix(h, w, C.byref(lp), C.byref(nr), C.byref(nhh)))
            rec["L"] = (np.ctypeslib.as_array(lp, shape=(nr.value, nhh.value)).copy() if nr.value
                        else np.zeros((0, nhh.value), np.float64))
        wins.append(rec)
    return dict(windows=wins, sites=_sites(h))


def call_windows(windows, want_L=False, want_site_reads=False, want_cigars=False, use_double=None):
    p = Prepared(windows)
    h = p.run(flags_of(want_L, want_site_reads, want_cigars, use_double))
    try:
        return results(h, p.n, want_L, want_cigars)
    finally:
        p.free(h)
