"""ctypes loader for the PairHMM oracle — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import
this module. It loads

* ``oracle/liboracle.so``  — our C restatement (pairhmm_oracle.c), and
* ``oracle/_ref/libref_pairhmm.so`` — the reference's AVX kernel compiled from
  /root/reference by oracle/Makefile (optional: absent when never built).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_SO = os.path.join(HERE, "liboracle.so")
REF_SO = os.path.join(HERE, "_ref", "libref_pairhmm.so")

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)


def build(ref: bool = True) -> None:
    """Compile the oracle (and the reference driver when sources exist)."""
    targets = ["oracle"] + (["ref"] if ref else [])
    subprocess.run(["make", "-s", "-C", HERE] + targets, check=True)


def _ptr(a, t):
    if a is None:
        return None
    return a.ctypes.data_as(t)


class _Lib:
    def __init__(self, path: str, prefix: str):
        self.path = path
        self.lib = C.CDLL(path)
        p = prefix
        self._f32 = getattr(self.lib, f"{p}_full_prob_f32")
        self._f64 = getattr(self.lib, f"{p}_full_prob_f64")
        self._pairs = getattr(self.lib, f"{p}_pairs")
        self._luts = getattr(self.lib, f"{p}_get_luts")
        self._sizes = getattr(self.lib, f"{p}_lut_sizes")
        args = [C.c_int, C.c_int] + [_u8p] * 6
        self._f32.argtypes = args
        self._f32.restype = C.c_float
        self._f64.argtypes = args
        self._f64.restype = C.c_double
        self._pairs.argtypes = [C.c_long, _i64p, _i32p, _i64p, _i32p] + [_u8p] * 6 + [
            _f32p, _f64p, _u8p, _f64p, C.c_int]
        self._pairs.restype = C.c_long
        self._luts.argtypes = [_f32p, _f64p, _f32p, _f64p, _f32p, _f64p]
        self._sizes.argtypes = [_i32p, _i32p, _i32p]

    def full_prob(self, rs: bytes, q: bytes, i: bytes, d: bytes, c: bytes, hap: bytes, f64=False):
        R, H = len(rs), len(hap)
        bufs = [np.frombuffer(x, dtype=np.uint8).copy() for x in (rs, q, i, d, c, hap)]
        fn = self._f64 if f64 else self._f32
        return fn(R, H, *[_ptr(b, _u8p) for b in bufs])

    def pairs(self, batch, nthreads: int = 1):
        """batch: dict from workloads (read_off, R, hap_off, H, rs, q, ins, dels, gcp, hap)."""
        n = len(batch["R"])
        raw32 = np.zeros(n, np.float32)
        raw64 = np.zeros(n, np.float64)
        resc = np.zeros(n, np.uint8)
        L = np.zeros(n, np.float64)
        b = batch
        nres = self._pairs(
            n, _ptr(b["read_off"], _i64p), _ptr(b["R"], _i32p), _ptr(b["hap_off"], _i64p),
            _ptr(b["H"], _i32p), _ptr(b["rs"], _u8p), _ptr(b["q"], _u8p), _ptr(b["ins"], _u8p),
            _ptr(b["dels"], _u8p), _ptr(b["gcp"], _u8p), _ptr(b["hap"], _u8p),
            _ptr(raw32, _f32p), _ptr(raw64, _f64p), _ptr(resc, _u8p), _ptr(L, _f64p), nthreads)
        return dict(raw_f32=raw32, raw_f64=raw64, rescued=resc, loglik=L, n_rescued=int(nres))

    def luts(self):
        n = [C.c_int32(), C.c_int32(), C.c_int32()]
        self._sizes(*[C.byref(x) for x in n])
        np_, nm, nj = (x.value for x in n)
        out = dict(ph2pr_f=np.zeros(np_, np.float32), ph2pr_d=np.zeros(np_, np.float64),
                   mm_f=np.zeros(nm, np.float32), mm_d=np.zeros(nm, np.float64),
                   jac_f=np.zeros(nj, np.float32), jac_d=np.zeros(nj, np.float64))
        self._luts(_ptr(out["ph2pr_f"], _f32p), _ptr(out["ph2pr_d"], _f64p),
                   _ptr(out["mm_f"], _f32p), _ptr(out["mm_d"], _f64p),
                   _ptr(out["jac_f"], _f32p), _ptr(out["jac_d"], _f64p))
        return out


class Oracle(_Lib):
    """Our C restatement (kind "port")."""

    def __init__(self, path: str = ORACLE_SO):
        if not os.path.exists(path):
            build(ref=False)
        super().__init__(path, "hco")
        self.lib.hco_finish.argtypes = [C.c_float, C.c_double]
        self.lib.hco_finish.restype = C.c_double
        self.lib.hco_normalize.argtypes = [C.c_int, C.c_int, _i32p, _f64p, _u8p]
        self.lib.hco_normalize.restype = C.c_int

    def finish(self, f: float, d: float) -> float:
        return self.lib.hco_finish(f, d)

    def normalize(self, L: np.ndarray, read_len: np.ndarray):
        L = np.ascontiguousarray(L, dtype=np.float64).copy()
        nr, nh = L.shape
        keep = np.zeros(nr, np.uint8)
        rl = np.ascontiguousarray(read_len, dtype=np.int32)
        self.lib.hco_normalize(nr, nh, _ptr(rl, _i32p), _ptr(L, _f64p), _ptr(keep, _u8p))
        return L, keep.astype(bool)


class Reference(_Lib):
    """The reference's own AVX kernel (kind "reference"); raises if not built."""

    def __init__(self, path: str = REF_SO):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        super().__init__(path, "ref")


def reference_available() -> bool:
    return os.path.exists(REF_SO)


# --------------------------------------------------------------------------
# Smith-Waterman: oracle/sw_oracle.c (kind "port", in
# liboracle.so) and the reference aligner (oracle/_ref/libref_sw.so).
REF_SW_SO = os.path.join(HERE, "_ref", "libref_sw.so")
SW_CIGAR_STRIDE = 4096


class _SWLib:
    def __init__(self, fn, nthreads_arg: bool):
        self._fn = fn
        self._nt = nthreads_arg
        args = [C.c_long, _i64p, _i32p, _u8p, _i64p, _i32p, _u8p] + [C.c_int] * 6 + [_i32p, C.c_char_p, C.c_int]
        fn.argtypes = args + ([C.c_int] if nthreads_arg else [])
        fn.restype = C.c_int

    def batch(self, b, params=(200, -150, -260, -11), overhang=9, shortcut=True, nthreads=1,
              stride=SW_CIGAR_STRIDE):
        """IntelSWAligner::align over a flat batch (sw_workloads layout).
        Returns (offsets int32[n], cigars list[str])."""
        n = len(b["ref_len"])
        off = np.zeros(n, np.int32)
        cig = C.create_string_buffer(max(1, n * stride))
        refs = b["refs"] if len(b["refs"]) else np.zeros(1, np.uint8)
        alts = b["alts"] if len(b["alts"]) else np.zeros(1, np.uint8)
        extra = [nthreads] if self._nt else []
        rc = self._fn(n, _ptr(b["ref_off"], _i64p), _ptr(b["ref_len"], _i32p), _ptr(refs, _u8p),
                      _ptr(b["alt_off"], _i64p), _ptr(b["alt_len"], _i32p), _ptr(alts, _u8p),
                      *params, overhang, int(bool(shortcut)), _ptr(off, _i32p), cig, stride, *extra)
        if rc != 0:
            raise RuntimeError("CIGAR buffer too small")
        raw = cig.raw
        cigars = [raw[k * stride:(k + 1) * stride].split(b"\0", 1)[0].decode() for k in range(n)]
        return off, cigars


class SWOracle(_SWLib):
    def __init__(self, path: str = ORACLE_SO):
        if not os.path.exists(path):
            build(ref=False)
        self.lib = C.CDLL(path)
        super().__init__(self.lib.hco_sw_batch, True)
        self.lib.hco_sw_align.argtypes = [C.c_int] * 4 + [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                                            C.c_char_p, C.c_int, _i32p]
        self.lib.hco_sw_align.restype = C.c_int

    def score(self, s1: bytes, s2: bytes, params=(200, -150, -260, -11), overhang=9) -> int:
        """The best end-point score of one pair's DP (hco_sw_align's *score)."""
        sc = C.c_int32()
        cig = C.create_string_buffer(SW_CIGAR_STRIDE * 4)
        self.lib.hco_sw_align(*params, s1, len(s1), s2, len(s2), overhang, cig, len(cig), C.byref(sc))
        return sc.value

    def scores(self, b, params=(200, -150, -260, -11), overhang=9, shortcut=True):
        """Per pair of a flat batch: score(), and 0 where the all-match
        shortcut answers the pair (shortcut on)."""
        out = np.zeros(len(b["ref_len"]), np.int32)
        for k in range(len(out)):
            r = b["refs"][b["ref_off"][k]:b["ref_off"][k] + b["ref_len"][k]].tobytes()
            a = b["alts"][b["alt_off"][k]:b["alt_off"][k] + b["alt_len"][k]].tobytes()
            if shortcut and self.lib.hco_sw_is_all_match(r, len(r), a, len(a)):
                continue
            out[k] = self.score(r, a, params, overhang)
        return out


class SWReference(_SWLib):
    def __init__(self, path: str = REF_SW_SO):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.lib = C.CDLL(path)
        super().__init__(self.lib.ref_sw_align_batch, False)


def sw_reference_available() -> bool:
    return os.path.exists(REF_SW_SO)


# --------------------------------------------------------------------------
# Genotyper numeric core: oracle/gt_oracle.c (in
# liboracle.so) and the reference's MathUtils (oracle/_ref/libref_math.so).
REF_MATH_SO = os.path.join(HERE, "_ref", "libref_math.so")


class GTOracle:
    def __init__(self, path: str = ORACLE_SO):
        if not os.path.exists(path):
            build(ref=False)
        self.lib = C.CDLL(path)
        self.lib.hco_approx_log10_sum_log10.argtypes = [C.c_double, C.c_double]
        self.lib.hco_approx_log10_sum_log10.restype = C.c_double
        self.lib.hco_gt_site.argtypes = [_f64p, C.c_int, _i32p, C.c_int, _i32p, C.c_int, _f64p, _i32p, _i32p]

    def approx(self, a: float, b: float) -> float:
        return self.lib.hco_approx_log10_sum_log10(a, b)

    def site(self, L, keep, hap_allele, n_alleles):
        L = np.ascontiguousarray(L, np.float64)
        keep = np.ascontiguousarray(keep, np.int32)
        amap = np.ascontiguousarray(hap_allele, np.int32)
        gl = np.zeros(n_alleles * (n_alleles + 1) // 2, np.float64)
        gi, gq = C.c_int32(), C.c_int32()
        self.lib.hco_gt_site(_ptr(L, _f64p), L.shape[1], _ptr(keep, _i32p), len(keep), _ptr(amap, _i32p),
                             n_alleles, _ptr(gl, _f64p), C.byref(gi), C.byref(gq))
        return gl, gi.value, gq.value


class MathReference:
    """The reference's MathUtils::approximate_log10_sum_log10, compiled in place."""

    def __init__(self, path: str = REF_MATH_SO):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.lib = C.CDLL(path)
        self.lib.ref_approx_log10_sum_log10.argtypes = [C.c_double, C.c_double]
        self.lib.ref_approx_log10_sum_log10.restype = C.c_double

    def approx(self, a: float, b: float) -> float:
        return self.lib.ref_approx_log10_sum_log10(a, b)


# --------------------------------------------------------------------------
# The reference's region chain compiled in place (oracle/_ref/libref_chain.so,
# oracle/ref_chain_driver.cpp): SAM parse, read filters and clipper, the
# aligner's front, IntelPairHMM::compute_likelihoods and the Genetyper.
REF_CHAIN_SO = os.path.join(HERE, "_ref", "libref_chain.so")
CHAIN_CONTIG = "c"   # the RNAME every read handed to the driver carries


class ReferenceThrew(Exception):
    """The reference threw a std::exception on this input."""


class _Blob:
    """Reader of the driver's blobs: little-endian int64 / double / length-prefixed bytes."""

    def __init__(self, raw: bytes):
        self.raw, self.at = raw, 0

    def i64(self) -> int:
        v = int.from_bytes(self.raw[self.at:self.at + 8], "little", signed=True)
        self.at += 8
        return v

    def u64(self) -> int:
        v = int.from_bytes(self.raw[self.at:self.at + 8], "little", signed=False)
        self.at += 8
        return v

    def f64s(self, n: int) -> np.ndarray:
        v = np.frombuffer(self.raw, np.float64, n, self.at).copy()
        self.at += 8 * n
        return v

    def i64s(self, n: int) -> np.ndarray:
        v = np.frombuffer(self.raw, np.int64, n, self.at).copy()
        self.at += 8 * n
        return v

    def bytes_(self) -> bytes:
        n = self.i64()
        v = self.raw[self.at:self.at + n]
        self.at += n
        return v

    def end(self):
        assert self.at == len(self.raw), (self.at, len(self.raw))


def sam_line(k, flag, pos, mapq, cigar, mate_same, seq, qual) -> str:
    """One read as the driver takes it: QNAME is the read's index, RNAME the driver's contig."""
    return "\t".join(str(x) for x in (k, flag, CHAIN_CONTIG, pos, mapq, cigar, "=" if mate_same else "chrOther", 0, 0,
                                      seq, qual))


def interval_sam(read_begin, read_end) -> str:
    """Reads of which only get_interval() matters (the genotyper's)."""
    return "\n".join(sam_line(k, 0, int(b) + 1, 60, f"{int(e) - int(b)}M", 1, "*", "*")
                     for k, (b, e) in enumerate(zip(read_begin, read_end)))


def haps_text(haps) -> str:
    """[{bases, begin, cigar}] (or bare bases, not aligned yet) as the driver takes them."""
    out = []
    for h in haps:
        if isinstance(h, (bytes, str)):
            h = dict(bases=h, begin=0, cigar="-")
        b = h["bases"].decode("latin-1") if isinstance(h["bases"], bytes) else h["bases"]
        out.append(f"{b} {h['begin']} {h['cigar']}")
    return "\n".join(out)


class ChainReference:
    """The hcr_* entries. Each returns plain Python / numpy data and raises
    ReferenceThrew where the reference threw."""

    THREW, SMALL, BAD_INPUT = -1, -2, -3

    def __init__(self, path: str = REF_CHAIN_SO):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.lib = L = C.CDLL(path)
        tail = [_u8p, C.c_long]
        L.hcr_parse.argtypes = [C.c_char_p, C.c_long] + tail
        L.hcr_prepare.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64] + tail
        L.hcr_align.argtypes = [C.c_char_p, C.c_long, C.c_char_p, C.c_long] + [C.c_int] * 4 + tail
        L.hcr_likelihoods.argtypes = [C.c_char_p, C.c_char_p] + tail
        L.hcr_normalize.argtypes = [C.c_char_p, C.c_long, _f64p] + tail
        L.hcr_normalize.restype = C.c_long
        L.hcr_gt_site.argtypes = [_f64p, C.c_long, C.c_long, _i32p, C.c_long, _i32p, C.c_long] + tail
        L.hcr_gt_site.restype = C.c_long
        L.hcr_genotype.argtypes = [C.c_char_p, C.c_char_p, _f64p, C.c_char_p, C.c_long] + [C.c_uint64] * 4 + tail
        L.hcr_chain.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_long] + [C.c_uint64] * 4 + tail
        for f in (L.hcr_parse, L.hcr_prepare, L.hcr_align, L.hcr_likelihoods, L.hcr_genotype, L.hcr_chain):
            f.restype = C.c_long

    def _call(self, fn, *args) -> _Blob:
        cap = 1 << 16
        while True:
            buf = np.zeros(cap, np.uint8)
            n = fn(*args, _ptr(buf, _u8p), cap)
            if n == self.SMALL:
                cap *= 8
                continue
            if n == self.THREW:
                raise ReferenceThrew()
            if n < 0:
                raise ValueError("input the reference driver refuses")
            return _Blob(buf[:n].tobytes())

    @staticmethod
    def _enc(s) -> bytes:
        return s if isinstance(s, bytes) else s.encode("latin-1")

    def parse(self, line):
        """dict(fail, FLAG, POS, MAPQ, elements [(length, op)], RNEXT, PNEXT, TLEN, SEQ, QUAL)."""
        raw = self._enc(line)
        b = self._call(self.lib.hcr_parse, raw, len(raw))
        out = dict(fail=b.i64(), FLAG=b.i64(), POS=b.i64(), MAPQ=b.i64())
        out["elements"] = [(b.u64(), chr(b.i64())) for _ in range(b.i64())]
        out.update(RNEXT=b.bytes_().decode("latin-1"), PNEXT=b.i64(), TLEN=b.i64(), SEQ=b.bytes_().decode("latin-1"),
                   QUAL=b.bytes_().decode("latin-1"))
        b.end()
        return out

    def prepare(self, sam: str, begin: int, end: int):
        """Per input read dict(reason, left (bool), and for a survivor POS, CIGAR, SEQ, QUAL)."""
        b = self._call(self.lib.hcr_prepare, self._enc(sam), begin, end)
        out = []
        for _ in range(b.i64()):
            r = dict(reason=b.i64(), left=not b.i64())
            if not r["left"]:
                r.update(POS=b.i64(), CIGAR=b.bytes_().decode(), SEQ=b.bytes_().decode("latin-1"),
                         QUAL=b.bytes_().decode("latin-1"))
            out.append(r)
        b.end()
        return out

    def align(self, ref, alt, params=(200, -150, -260, -11)):
        ref, alt = self._enc(ref), self._enc(alt)
        b = self._call(self.lib.hcr_align, ref, len(ref), alt, len(alt), *params)
        out = (b.u64(), b.bytes_().decode())
        b.end()
        return out

    def likelihoods(self, sam: str, haps):
        """dict(raw (reads x haps, before normalisation), kept (indices), L (kept x haps))."""
        b = self._call(self.lib.hcr_likelihoods, self._enc(sam), self._enc(haps_text(haps)))
        nr, nh = b.i64(), b.i64()
        raw = b.f64s(nr * nh).reshape(nr, nh)
        nk = b.i64()
        kept = b.i64s(nk)
        L = b.f64s(nk * nh).reshape(nk, nh)
        b.end()
        return dict(raw=raw, kept=kept, L=L)

    def normalize(self, L, read_len):
        """normalize_likelihoods_and_filter_poorly_modeled_reads on a matrix handed in: (kept indices, L left)."""
        L = np.ascontiguousarray(L, np.float64)
        sam = "\n".join(sam_line(k, 0, 1, 60, f"{int(n)}M", 1, "A" * int(n), "I" * int(n)) for k, n in enumerate(read_len))
        b = self._call(self.lib.hcr_normalize, self._enc(sam), L.shape[1], _ptr(L, _f64p))
        nk = b.i64()
        kept = b.i64s(nk)
        out = b.f64s(nk * L.shape[1]).reshape(nk, L.shape[1])
        b.end()
        return kept, out

    def site(self, L, keep, hap_allele, n_alleles):
        """One site's arithmetic, as GTOracle.site: (genotype likelihoods, index, quality)."""
        L = np.ascontiguousarray(L, np.float64)
        keep = np.ascontiguousarray(keep, np.int32)
        amap = np.ascontiguousarray(hap_allele, np.int32)
        b = self._call(self.lib.hcr_gt_site, _ptr(L, _f64p), L.shape[0], L.shape[1], _ptr(keep, _i32p), len(keep),
                       _ptr(amap, _i32p), n_alleles)
        out = (b.f64s(n_alleles * (n_alleles + 1) // 2), b.i64(), b.i64())
        b.end()
        return out

    @staticmethod
    def _variants(b: _Blob):
        out = []
        for _ in range(b.i64()):
            v = dict(begin=b.u64(), end=b.u64())
            v["alleles"] = [b.bytes_() for _ in range(b.i64())]
            v.update(a1=b.i64(), a2=b.i64(), gq=b.i64(), text=b.bytes_().decode("latin-1"))
            out.append(v)
        return out

    def genotype(self, region):
        """A region in hcgt.call_regions' layout. dict(threw, variants, sites):
        `threw` / `variants` are assign_genotype_likelihoods' own outcome; `sites`
        has, per events_begins entry inside the origin, dict(begin, threw) and,
        where the site did not throw, loc_begin, loc_end, alleles and (for at most
        7 alleles) hap_allele, keep, genotype_likelihoods, genotype_index,
        genotype_quality."""
        L = np.ascontiguousarray(region["L"], np.float64)
        ref = self._enc(region["ref"])
        pb = int(region["padded_begin"])
        b = self._call(self.lib.hcr_genotype, self._enc(interval_sam(region["read_begin"], region["read_end"])),
                       self._enc(haps_text(region["haps"])), _ptr(L if L.size else np.zeros(1), _f64p), ref, len(ref),
                       pb, pb + len(ref), int(region["origin_begin"]), int(region["origin_end"]))
        out = dict(threw=bool(b.i64()), variants=[], sites=[])
        if not out["threw"]:
            out["variants"] = self._variants(b)
        nh = len(region["haps"])
        for _ in range(b.i64()):
            s = dict(begin=b.u64(), threw=bool(b.i64()))
            if not s["threw"]:
                s.update(loc_begin=b.u64(), loc_end=b.u64())
                s["alleles"] = [b.bytes_() for _ in range(b.i64())]
                A = len(s["alleles"])
                if A <= 7:
                    s["hap_allele"] = b.i64s(nh).astype(np.int32)
                    s["keep"] = b.i64s(b.i64()).astype(np.int32)
                    s["genotype_likelihoods"] = b.f64s(A * (A + 1) // 2)
                    s.update(genotype_index=b.i64(), genotype_quality=b.i64())
            out["sites"].append(s)
        b.end()
        return out

    def chain(self, sam: str, haps, ref, padded_begin, origin_begin, origin_end):
        """dict(outcome (0 called, 1 no reads left, 2 at most one haplotype), n_reads, variants)."""
        ref = self._enc(ref)
        b = self._call(self.lib.hcr_chain, self._enc(sam), self._enc(haps_text(haps)), ref, len(ref), padded_begin,
                       padded_begin + len(ref), origin_begin, origin_end)
        out = dict(outcome=b.i64(), n_reads=0, variants=[])
        if out["outcome"] == 0:
            out["n_reads"] = b.i64()
            out["variants"] = self._variants(b)
        b.end()
        return out


def chain_reference_available() -> bool:
    return os.path.exists(REF_CHAIN_SO)


# --------------------------------------------------------------------------
# The reference's assembler compiled in place (oracle/_ref/libref_asm.so,
# oracle/ref_asm_driver.cpp): Assembler::assemble over GraphWrapper, with
# oracle/boost_standin/boost/graph/ for the container and the DFS.
REF_ASM_SO = os.path.join(HERE, "_ref", "libref_asm.so")


class AsmReference:
    """hcr_asm. assemble() returns the record the asm fixture keeps: status,
    kmer_size, attempts (the codes of include/hc_asm.h), unique (the unique
    k-mer count of every attempt that built a graph), n_paths, haps [(bases,
    score)] in the reference's order, source, sink and edges [(from, to, last
    byte, count, is_ref, is_on_path, creation index)] of the accepted graph.
    Raises ReferenceThrew where the reference threw."""

    SMALL = -2

    def __init__(self, path: str = REF_ASM_SO):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.lib = C.CDLL(path)
        self.lib.hcr_asm.argtypes = [C.c_char_p, C.c_long, C.c_long, _i64p, _i32p, _u8p, _u8p, _u8p, C.c_long]
        self.lib.hcr_asm.restype = C.c_long

    def assemble(self, reads, ref: bytes):
        lens = np.array([len(b) for b, _ in reads], np.int32)
        offs = np.zeros(len(reads), np.int64)
        if len(reads):
            offs[1:] = np.cumsum(lens[:-1])
        bases = np.frombuffer(b"".join(b for b, _ in reads) + b"\0", np.uint8).copy()
        quals = np.frombuffer(b"".join(q for _, q in reads) + b"\0", np.uint8).copy()
        cap = 1 << 20
        while True:
            buf = np.zeros(cap, np.uint8)
            n = self.lib.hcr_asm(ref, len(ref), len(reads), _ptr(offs if len(reads) else np.zeros(1, np.int64), _i64p),
                                 _ptr(lens if len(reads) else np.zeros(1, np.int32), _i32p), _ptr(bases, _u8p),
                                 _ptr(quals, _u8p), _ptr(buf, _u8p), cap)
            if n == self.SMALL:
                cap *= 8
                continue
            break
        b = _Blob(buf[:n].tobytes())
        if b.i64():
            raise ReferenceThrew()
        haps = []
        for _ in range(b.i64()):
            bases_ = b.bytes_()
            haps.append((bases_, float(b.f64s(1)[0])))
        att = b.i64s(18).reshape(9, 2)
        out = dict(attempts=att[:, 0].tolist(), unique=att[:, 1].tolist(), haps=haps, kmer_size=b.i64(), n_paths=b.i64(),
                   source=b.i64(), sink=b.i64())
        ne = b.i64()
        out["edges"] = [tuple(row) for row in b.i64s(7 * ne).reshape(ne, 7).tolist()]
        out["status"] = 0 if haps else 1   # HC_ASM_OK / HC_ASM_NO_HAPLOTYPES
        b.end()
        return out


def asm_reference_available() -> bool:
    return os.path.exists(REF_ASM_SO)
