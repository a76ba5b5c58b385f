"""Python mirror of the MI355X assembler (include/hc_asm.h).

``assemble(regions, want_graph=False)`` is one hc_asm_assemble: Assembler::
assemble (reference assembler/assembler.hpp:56-68) for every region in one
device pass. A region is a dict {ref: bytes, reads: [(bases, quals), ...]}.
Returns one dict per region: ``status`` (OK, NO_HAPLOTYPES, TOO_COMPLEX),
``kmer_size``, ``attempts`` (nine outcome codes), ``n_paths``, ``haps``
[(bases, score)] in final order, and with want_graph ``graph`` (the on-path
edges (from, to, base, count, is_ref, seq) in creation order), ``source`` and
``sink``. The haplotype bases go to hcregion.call_regions as they are (aligned
on the device). No CPU path: raises AsmError without the library or a gfx950
device.
"""
from __future__ import annotations

import ctypes as C

import hcbind
import hcphmm
from hcbind import f64p as _f64p, i32p as _i32p, i64p as _i64p, u8p as _u8p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_asm.h")
OK, NO_HAPLOTYPES, TOO_COMPLEX = 0, 1, 2
NOT_TRIED, SHORT_REF, TOO_MANY_KMERS, CYCLE, ACCEPTED = 0, 1, 2, 3, 4
WANT_GRAPH = 1
MAX_ATTEMPTS, MAX_HAPS, MAX_PATHS, MAX_REGION_READ_BASES, MAX_GRAPH_EDGES = 9, 128, 65536, 131072, 16384


class AsmError(hcbind.Error):
    prefix = "hc_asm"


class Read(C.Structure):
    _fields_ = [("bases", C.c_char_p), ("quals", C.c_char_p), ("length", C.c_int32)]


class Region(C.Structure):
    _fields_ = [("ref", C.c_char_p), ("ref_len", C.c_int32), ("reads", C.POINTER(Read)), ("n_reads", C.c_int32)]


class Edge(C.Structure):
    _fields_ = [("frm", C.c_int32), ("to", C.c_int32), ("count", C.c_int32), ("seq", C.c_int32),
                ("base", C.c_uint8), ("is_ref", C.c_uint8), ("reserved", C.c_uint16)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hcphmm.lib()
        hcphmm.check_build_id()   # a stale binary would not have these entry points, or other ones
        vp = C.c_void_p
        L.hc_asm_assemble.argtypes = [C.POINTER(Region), C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.hc_asm_result_region.argtypes = [vp, C.c_int32, _i32p, _i32p, C.POINTER(_u8p), _i32p, _i64p]
        L.hc_asm_result_hap.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(_u8p), _i32p, _f64p]
        L.hc_asm_result_graph.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(Edge)), _i32p, _i32p, _i32p]
        L.hc_asm_result_free.argtypes = [vp]
        L.hcx_asm_paths_from_graph.argtypes = [C.c_char_p, C.c_int32, C.POINTER(Edge), C.c_int32, C.c_int32,
                                               C.c_int32, C.POINTER(vp)]   # test hook
        _lib = L
    return _lib


def declared_symbols(header: str = HEADER):
    return hcbind.declared(header, "hc_asm_")


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, AsmError)


class Prepared:
    """The C structs of a call, built once (timing tools time run() alone)."""

    def __init__(self, regions):
        self.n = len(regions)
        self.arr = (Region * max(self.n, 1))()
        self.keep_alive = []
        for k, r in enumerate(regions):
            reads = r["reads"]
            ra = (Read * max(len(reads), 1))()
            for j, (b, q) in enumerate(reads):
                if q is not None and len(q) != len(b):
                    raise AsmError(hcphmm.EINVAL, f"region {k} read {j}: {len(b)} bases, {len(q)} qualities")
                ra[j] = Read(b, q, len(b))
            self.keep_alive.append(ra)
            ref = r["ref"]
            self.arr[k] = Region(ref, 0 if ref is None else len(ref), ra if len(reads) else None, len(reads))

    def run(self, want_graph=False):
        """One hc_asm_assemble; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_asm_assemble(self.arr, self.n, WANT_GRAPH if want_graph else 0, C.byref(h)))
        return h

    @staticmethod
    def free(h):
        lib().hc_asm_result_free(h)


def records(h, n, want_graph=False):
    """The regions of a result handle as dicts."""
    L = lib()
    out = []
    for r in range(n):
        status, k, nh, npaths = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        att = _u8p()
        _check(L.hc_asm_result_region(h, r, C.byref(status), C.byref(k), C.byref(att), C.byref(nh), C.byref(npaths)))
        rec = dict(status=status.value, kmer_size=k.value, attempts=[int(att[t]) for t in range(MAX_ATTEMPTS)],
                   n_paths=npaths.value, haps=[])
        for j in range(nh.value):
            b, ln, sc = _u8p(), C.c_int32(), C.c_double()
            _check(L.hc_asm_result_hap(h, r, j, C.byref(b), C.byref(ln), C.byref(sc)))
            rec["haps"].append((C.string_at(b, ln.value), sc.value))
        if want_graph:
            e, ne, src, snk = C.POINTER(Edge)(), C.c_int32(), C.c_int32(), C.c_int32()
            _check(L.hc_asm_result_graph(h, r, C.byref(e), C.byref(ne), C.byref(src), C.byref(snk)))
            rec.update(graph=[(e[i].frm, e[i].to, e[i].base, e[i].count, e[i].is_ref, e[i].seq)
                              for i in range(ne.value)], source=src.value, sink=snk.value)
        out.append(rec)
    return out


def assemble(regions, want_graph=False):
    p = Prepared(regions)
    h = p.run(want_graph)
    try:
        return records(h, p.n, want_graph)
    finally:
        p.free(h)


def paths_from_graph(source_kmer: bytes, edges, source: int, sink: int):
    """The host half alone (test hook hcx_asm_paths_from_graph): edges are
    (from, to, base, count, is_ref, seq) in creation order. Returns one region dict."""
    arr = (Edge * max(len(edges), 1))()
    for i, (u, v, base, count, is_ref, seq) in enumerate(edges):
        arr[i] = Edge(u, v, count, seq, base, is_ref, 0)
    h = C.c_void_p()
    _check(lib().hcx_asm_paths_from_graph(source_kmer, len(source_kmer), arr, len(edges), source, sink, C.byref(h)))
    try:
        return records(h, 1, True)[0]
    finally:
        lib().hc_asm_result_free(h)
