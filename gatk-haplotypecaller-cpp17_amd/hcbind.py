"""What the Python mirrors of the C headers share (hcphmm, hcsw, hcgt, hcregion,
hcasm, hcprep, hccall, hccontig, hcgenome, hcbam, hcintervals): the pointer types, the base of their error
classes, the header / binding symbol lists of the export tests, the return code
check and the conversion of hc_gt_call_site records to dicts.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)


class Error(RuntimeError):
    """``<prefix> error <code>: <msg>``; a mirror's error class sets ``prefix``."""
    prefix = "hc"

    def __init__(self, code: int, msg: str):
        super().__init__(f"{self.prefix} error {code}: {msg}")
        self.code = code
        self.msg = msg


class CallSite(C.Structure):
    """hc_gt_call_site (include/hc_gt.h)."""
    _fields_ = [("region", C.c_int32), ("status", C.c_int32), ("begin", C.c_int64), ("loc_end", C.c_int64),
                ("n_alleles", C.c_int32), ("n_haps", C.c_int32), ("alleles", C.POINTER(C.c_char_p)),
                ("hap_allele", i32p), ("keep", i32p), ("n_keep", C.c_int32), ("n_genotypes", C.c_int32),
                ("genotype_likelihoods", f64p), ("genotype_index", C.c_int32), ("a1", C.c_int32),
                ("a2", C.c_int32), ("genotype_quality", C.c_int32)]


def declared(header: str, prefix_regex: str):
    """The functions named <prefix_regex>... that a C header declares."""
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(%s\w+)\s*\(" % prefix_regex, open(header).read(), re.M)))


def mirrored(lib, symbols):
    """Those of `symbols` that `lib` binds with argtypes (for the export tests)."""
    return sorted(s for s in symbols if getattr(getattr(lib, s), "argtypes", None) is not None)


def check(rc: int, error):
    """Raises error(rc, the library's message) unless rc is 0."""
    if rc != 0:
        import hcphmm   # (imports this module)
        msg = hcphmm.lib().hc_phmm_last_error()
        raise error(rc, msg.decode() if msg else "")


def call_sites(handle, accessor, check, keep_counts=True):
    """The hc_gt_call_site records of a result handle as dicts. keep_counts adds
    ``keep_is_null`` and ``n_keep`` (the callers whose read lists are on request)."""
    sites, n = C.POINTER(CallSite)(), C.c_int64()
    check(accessor(handle, C.byref(sites), C.byref(n)))
    out = []
    for k in range(n.value):
        s = sites[k]
        d = dict(
            region=s.region, status=s.status, begin=s.begin, loc_end=s.loc_end, n_alleles=s.n_alleles,
            alleles=[s.alleles[j] for j in range(s.n_alleles)] if s.alleles else [],
            hap_allele=np.array(s.hap_allele[:s.n_haps], np.int32) if s.hap_allele else np.zeros(0, np.int32),
            keep=np.array(s.keep[:s.n_keep], np.int32) if s.n_keep else np.zeros(0, np.int32),
            genotype_likelihoods=np.array(s.genotype_likelihoods[:s.n_genotypes], np.float64)
            if s.genotype_likelihoods else np.zeros(0, np.float64),
            genotype_index=s.genotype_index, a1=s.a1, a2=s.a2, genotype_quality=s.genotype_quality)
        if keep_counts:
            d.update(keep_is_null=not bool(s.keep), n_keep=s.n_keep)
        out.append(d)
    return out
