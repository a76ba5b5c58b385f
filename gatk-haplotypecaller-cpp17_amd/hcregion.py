"""Python mirror of the MI355X region caller (include/hc_region.h).

``call_regions(regions)`` is one hc_region_call: the haplotypes of every region
are aligned against its window, reads x haplotypes go through the PairHMM, the
poorly modelled reads are filtered and the kept reads are genotyped, with both
hand-offs on the device. Regions are dicts in the region_workloads layout
{ref, padded_begin, origin_begin, origin_end, haps, reads, read_begin,
read_end}; a haplotype is its bases (aligned on the device) or a dict {bases,
begin, cigar}. Returns a dict: ``sites`` (records as hcgt.call_regions gives
them), ``keep`` (per region, one bool per read), and on request ``L`` (per
region, kept reads x haplotypes) and ``alignments`` (per region, (begin, cigar)
per haplotype). No CPU path: raises RegionError without the library or a gfx950
device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hcbind
import hcgt
import hcphmm
from hcbind import f64p as _f64p, i32p as _i32p, i64p as _i64p, u8p as _u8p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_region.h")
F64, DEFAULT_MODE, WANT_L, WANT_SITE_READS, WANT_CIGARS = 1, 2, 16, 32, 64


class RegionError(hcbind.Error):
    prefix = "hc_region"


class Hap(C.Structure):
    _fields_ = [("bases", C.c_char_p), ("length", C.c_int32), ("alignment_begin", C.c_int32), ("cigar", C.c_char_p)]


class RegionIn(C.Structure):
    _fields_ = [("ref", C.c_char_p), ("ref_len", C.c_int32), ("padded_begin", C.c_int64),
                ("origin_begin", C.c_int64), ("origin_end", C.c_int64), ("haps", C.POINTER(Hap)),
                ("n_haps", C.c_int32), ("reads", C.POINTER(hcphmm.Read)), ("read_begin", _i64p),
                ("read_end", _i64p), ("n_reads", C.c_int32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hcgt.lib()
        vp = C.c_void_p
        L.hc_region_call.argtypes = [C.POINTER(RegionIn), C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.hc_region_calls_sites.argtypes = [vp, C.POINTER(C.POINTER(hcgt.CallSite)), _i64p]
        L.hc_region_calls_reads.argtypes = [vp, C.c_int32, C.POINTER(_u8p), _i32p, _i32p]
        L.hc_region_calls_matrix.argtypes = [vp, C.c_int32, C.POINTER(_f64p), _i32p, _i32p]
        L.hc_region_calls_alignment.argtypes = [vp, C.c_int32, C.c_int32, _i32p, C.POINTER(C.c_char_p)]
        L.hc_region_calls_free.argtypes = [vp]
        L.hcx_region_finish.argtypes = [_f64p, C.c_int32, _i32p, _i32p, _i32p, _f64p, _u8p, _i32p, _i64p]   # test hook
        _lib = L
    return _lib


def declared_symbols(header: str = HEADER):
    return hcbind.declared(header, "hc_region_")


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, RegionError)


def flags_of(want_L=False, want_site_reads=False, want_cigars=False, use_double=None) -> int:
    """use_double: None = the process default (hcphmm.init); True / False = this call's mode."""
    f = DEFAULT_MODE if use_double is None else (F64 if use_double else 0)
    return f | (WANT_L if want_L else 0) | (WANT_SITE_READS if want_site_reads else 0) | \
        (WANT_CIGARS if want_cigars else 0)


class Prepared:
    """The C structs of a call, built once (timing tools time run() alone)."""

    def __init__(self, regions):
        self.n = len(regions)
        self.arr = (RegionIn * max(self.n, 1))()
        self.keep_alive = []
        self.shapes = []
        for k, r in enumerate(regions):
            haps = (Hap * max(len(r["haps"]), 1))()
            for j, h in enumerate(r["haps"]):
                if isinstance(h, dict):
                    cig = h["cigar"]
                    haps[j] = Hap(h["bases"], len(h["bases"]), int(h["begin"]),
                                  None if cig is None else cig.encode())
                else:
                    haps[j] = Hap(h, len(h), 0, None)
            ra, _ha, kk = hcphmm._structs(r["reads"], [])
            rb = np.ascontiguousarray(r["read_begin"], np.int64)
            re_ = np.ascontiguousarray(r["read_end"], np.int64)
            nr = len(r["reads"])
            self.keep_alive += [haps, ra, kk, rb, re_]
            self.shapes.append((nr, len(r["haps"])))
            ref = r["ref"]
            self.arr[k] = RegionIn(ref, 0 if ref is None else len(ref), int(r["padded_begin"]),
                                   int(r["origin_begin"]), int(r["origin_end"]), haps, len(r["haps"]),
                                   ra if nr else None, rb.ctypes.data_as(_i64p) if len(rb) else None,
                                   re_.ctypes.data_as(_i64p) if len(re_) else None, nr)

    def run(self, flags: int):
        """One hc_region_call; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_region_call(self.arr, self.n, flags, C.byref(h)))
        return h

    @staticmethod
    def free(h):
        lib().hc_region_calls_free(h)

    @staticmethod
    def sites(h):
        return hcbind.call_sites(h, lib().hc_region_calls_sites, _check)

    def keep(self, h, region: int):
        p, nr, nk = _u8p(), C.c_int32(), C.c_int32()
        _check(lib().hc_region_calls_reads(h, region, C.byref(p), C.byref(nr), C.byref(nk)))
        k = np.array(p[:nr.value], np.uint8).astype(bool) if nr.value else np.zeros(0, bool)
        assert int(k.sum()) == nk.value
        return k

    def matrix(self, h, region: int):
        p, nk, nh = _f64p(), C.c_int32(), C.c_int32()
        _check(lib().hc_region_calls_matrix(h, region, C.byref(p), C.byref(nk), C.byref(nh)))
        if nk.value == 0:
            return np.zeros((0, nh.value), np.float64)
        return np.ctypeslib.as_array(p, shape=(nk.value, nh.value)).copy()

    def alignment(self, h, region: int, hap: int):
        b, c = C.c_int32(), C.c_char_p()
        _check(lib().hc_region_calls_alignment(h, region, hap, C.byref(b), C.byref(c)))
        return b.value, c.value.decode()


def call_regions(regions, want_L=False, want_site_reads=False, want_cigars=False, use_double=None):
    p = Prepared(regions)
    h = p.run(flags_of(want_L, want_site_reads, want_cigars, use_double))
    try:
        out = dict(sites=p.sites(h), keep=[p.keep(h, r) for r in range(p.n)])
        if want_L:
            out["L"] = [p.matrix(h, r) for r in range(p.n)]
        if want_cigars:
            out["alignments"] = [[p.alignment(h, r, j) for j in range(nh)] if not isinstance(regions[r]["haps"][0], dict)
                                 else None for r, (_nr, nh) in enumerate(p.shapes)]
        return out
    finally:
        p.free(h)


def finish(mats, read_lens):
    """Test hook: region_finish_* alone. mats: one (n_reads, n_haps) float64 array
    per region; read_lens: one int array per region. Returns per region
    (capped kept rows, keep flags, indices of the kept reads as the compacted
    intervals carry them)."""
    n = len(mats)
    mats = [np.ascontiguousarray(m, np.float64) for m in mats]
    nr = np.array([m.shape[0] for m in mats], np.int32)
    nh = np.array([m.shape[1] for m in mats], np.int32)
    L = np.concatenate([m.ravel() for m in mats]) if n else np.zeros(0)
    L = np.ascontiguousarray(np.concatenate([L, np.zeros(1)]))
    rl = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).ravel() for x in read_lens] + [np.zeros(1, np.int32)]),
                              np.int32)
    total = int(nr.sum())
    Lo = np.zeros(len(L), np.float64)
    keep = np.zeros(total + 1, np.uint8)
    nk = np.zeros(max(n, 1), np.int32)
    order = np.zeros(total + 1, np.int64)
    _check(lib().hcx_region_finish(L.ctypes.data_as(_f64p), n, nr.ctypes.data_as(_i32p), nh.ctypes.data_as(_i32p),
                                   rl.ctypes.data_as(_i32p), Lo.ctypes.data_as(_f64p), keep.ctypes.data_as(_u8p),
                                   nk.ctypes.data_as(_i32p), order.ctypes.data_as(_i64p)))
    out, lo, ro = [], 0, 0
    for r in range(n):
        k = int(nk[r])
        out.append((Lo[lo:lo + k * nh[r]].reshape(k, nh[r]).copy(), keep[ro:ro + nr[r]].astype(bool),
                    order[ro:ro + nr[r]].copy()))
        lo += int(nr[r]) * int(nh[r])
        ro += int(nr[r])
    return out
