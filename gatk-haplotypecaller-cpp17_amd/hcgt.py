"""Python mirror of the MI355X genotyper numeric core (include/hc_gt.h).

``genotype_sites(mats, sites)`` is the per-site arithmetic of
Genetyper::assign_genotype_likelihoods (reference genotyper/genotyper.hpp:369-399:
marginalize -> calculate_genotype_likelihoods -> get_genotype_quality_and_max_
genotype_index) for many sites in one device pass. Sites are dicts
{m: matrix index, keep: int32[], hap_allele: int32[], n_alleles} over the
read-major likelihood matrices ``mats`` (gt_workloads layout). Returns a list of
(genotype_likelihoods float64[], genotype_index, genotype_quality).
No CPU path: raises GTError without the library or a gfx950 device.

``call_regions(regions)`` is the whole of assign_genotype_likelihoods: regions
in (gt_workloads.regions layout), one dict per in-origin site out, with the
events, alleles, haplotype -> allele map and kept reads computed on the device
ahead of the same arithmetic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import hcbind
import hcphmm
from hcbind import CallSite, f64p as _f64p, i32p as _i32p, i64p as _i64p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_gt.h")


class GTError(hcbind.Error):
    prefix = "hc_gt"


class Site(C.Structure):
    _fields_ = [("L", _f64p), ("n_reads", C.c_int32), ("n_haps", C.c_int32), ("keep", _i32p),
                ("n_keep", C.c_int32), ("hap_allele", _i32p), ("n_alleles", C.c_int32),
                ("genotype_likelihoods", _f64p), ("genotype_index", _i32p), ("genotype_quality", _i32p)]


class HapAln(C.Structure):
    _fields_ = [("bases", C.c_char_p), ("length", C.c_int32), ("alignment_begin", C.c_int32), ("cigar", C.c_char_p)]


class Region(C.Structure):
    _fields_ = [("ref", C.c_char_p), ("ref_len", C.c_int32), ("padded_begin", C.c_int64),
                ("origin_begin", C.c_int64), ("origin_end", C.c_int64), ("haps", C.POINTER(HapAln)),
                ("n_haps", C.c_int32), ("read_begin", _i64p), ("read_end", _i64p), ("n_reads", C.c_int32),
                ("L", _f64p)]


EMITTED, HOM_REF, LOW_QUALITY_HET, TOO_MANY_ALLELES = 0, 1, 2, 3
MAX_HAPS, MAX_REF_LEN, MAX_HAP_LEN = 128, 1023, 1024

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hcphmm.lib()
        L.hc_gt_genotype_sites.argtypes = [C.POINTER(Site), C.c_int32]
        L.hc_gt_call_regions.argtypes = [C.POINTER(Region), C.c_int32, C.POINTER(C.c_void_p)]
        L.hc_gt_calls_sites.argtypes = [C.c_void_p, C.POINTER(C.POINTER(CallSite)), _i64p]
        L.hc_gt_calls_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def declared_symbols(header: str = HEADER):
    return hcbind.declared(header, "hc_gt_")


def _check(rc: int):
    hcbind.check(rc, GTError)


class Prepared:
    """The C structs of a call, built once (the bench times run() alone)."""

    def __init__(self, mats, sites):
        self.mats = [np.ascontiguousarray(m, np.float64) for m in mats]
        self.n = len(sites)
        self.arr = (Site * max(self.n, 1))()
        self.keep_alive, self.outs = [], []
        for k, s in enumerate(sites):
            m = self.mats[s["m"]]
            keep = np.ascontiguousarray(s["keep"], np.int32)
            amap = np.ascontiguousarray(s["hap_allele"], np.int32)
            A = int(s["n_alleles"])
            gl = np.zeros(A * (A + 1) // 2, np.float64)
            gi = np.zeros(1, np.int32)
            gq = np.zeros(1, np.int32)
            self.keep_alive += [keep, amap]
            self.outs.append((gl, gi, gq))
            self.arr[k] = Site(m.ctypes.data_as(_f64p), m.shape[0], m.shape[1],
                               keep.ctypes.data_as(_i32p) if len(keep) else None, len(keep),
                               amap.ctypes.data_as(_i32p), A, gl.ctypes.data_as(_f64p),
                               gi.ctypes.data_as(_i32p), gq.ctypes.data_as(_i32p))

    def run(self):
        _check(lib().hc_gt_genotype_sites(self.arr, self.n))

    def results(self):
        return [(gl.copy(), int(gi[0]), int(gq[0])) for gl, gi, gq in self.outs]


def genotype_sites(mats, sites):
    p = Prepared(mats, sites)
    p.run()
    return p.results()


class PreparedRegions:
    """The C structs of a call_regions call, built once (timing tools time run() alone)."""

    def __init__(self, regions):
        self.n = len(regions)
        self.arr = (Region * max(self.n, 1))()
        self.keep_alive = []
        for k, r in enumerate(regions):
            haps = (HapAln * max(len(r["haps"]), 1))()
            for j, h in enumerate(r["haps"]):
                haps[j] = HapAln(h["bases"], len(h["bases"]), int(h["begin"]), h["cigar"].encode())
            rb = np.ascontiguousarray(r["read_begin"], np.int64)
            re_ = np.ascontiguousarray(r["read_end"], np.int64)
            L = np.ascontiguousarray(r["L"], np.float64)
            self.keep_alive += [haps, rb, re_, L]
            self.arr[k] = Region(r["ref"], len(r["ref"]), int(r["padded_begin"]), int(r["origin_begin"]),
                                 int(r["origin_end"]), haps, len(r["haps"]),
                                 rb.ctypes.data_as(_i64p) if len(rb) else None,
                                 re_.ctypes.data_as(_i64p) if len(re_) else None, len(rb),
                                 L.ctypes.data_as(_f64p) if L.size else None)

    def run(self):
        """One hc_gt_call_regions; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_gt_call_regions(self.arr, self.n, C.byref(h)))
        return h

    @staticmethod
    def free(h):
        lib().hc_gt_calls_free(h)

    @staticmethod
    def records(h):
        return hcbind.call_sites(h, lib().hc_gt_calls_sites, _check, keep_counts=False)


def call_regions(regions):
    """Site records (dicts) of every region: region, status, begin, loc_end,
    n_alleles, alleles (bytes), hap_allele, keep, genotype_likelihoods,
    genotype_index, a1, a2, genotype_quality."""
    p = PreparedRegions(regions)
    h = p.run()
    try:
        return p.records(h)
    finally:
        p.free(h)
