"""Python mirror of the interval calls of the MI355X genome caller
(include/hc_intervals.h).

``call_genome(sam, contigs, intervals, ...)`` is one hc_genome_call_intervals
and ``call_genome_bam(bam, contigs, intervals, index=None, ...)`` one
hc_bam_genome_call_intervals: the arguments of hcgenome.call_genome and
hcbam.call_genome_bam plus ``intervals``, a list of (contig, begin, end) with
``contig`` a table index or a name of the table and [begin, end) 0-based and
half-open. Both return the dict of hcgenome.results plus ``merged`` (the merged
intervals as (contig index, begin, end), sorted) and ``asked`` (the asked
genome-wide windows, ascending); the BAM call adds ``bases``. A window that is
not asked has status NOT_ASKED. ``index`` is the bytes of the file's .bai: with
it only the members that hold the asked ranges are uploaded and inflated, and
``index_stats`` (chunks, members, bytes_up, records; all 0 without an index)
says how many; the records of the result are then those framed from the chosen
chunks.

``parse_bed(text, names)`` reads the first three white-space separated columns
of a BED text into such a list: empty lines and lines that begin with ``#``,
``track`` or ``browser`` are skipped, a name outside ``names`` or a line with
fewer than three columns is a ValueError naming the 1-based line.

No CPU path: raises IntervalError without the library or a gfx950 device.
"""
from __future__ import annotations

import ctypes as C

import hcbam
import hcbind
import hcgenome
import hcphmm
from hcbind import i32p as _i32p

HEADER = hcphmm.HEADER.replace("hc_pairhmm.h", "hc_intervals.h")
NOT_ASKED = 3


class IntervalError(hcbam.BamError):
    prefix = "hc_intervals"


class Interval(C.Structure):
    """hc_interval."""
    _fields_ = [("contig", C.c_int32), ("begin", C.c_int64), ("end", C.c_int64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = hcbam.lib()
        vp = C.c_void_p
        tail = [C.POINTER(hcgenome.Contig), C.c_int32, C.POINTER(Interval), C.c_int32, C.c_int32, C.c_int32, C.c_uint64,
                C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.hc_genome_call_intervals.argtypes = [C.c_char_p, C.c_int64] + tail
        L.hc_bam_genome_call_intervals.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64] + tail
        L.hc_genome_result_intervals.argtypes = [vp, C.POINTER(C.POINTER(Interval)), _i32p, C.POINTER(_i32p), _i32p]
        L.hc_bam_genome_result_index.argtypes = [vp, _i32p, _i32p, hcbind.i64p, hcbind.i64p]
        _lib = L
    return _lib


def declared_symbols():
    """The entry points of hc_intervals.h."""
    return hcbind.declared(HEADER, "hc_(?:bam_)?genome_")


def mirrored_symbols():
    """The entry points this module binds (for the export test)."""
    return hcbind.mirrored(lib(), declared_symbols())


def _check(rc: int):
    hcbind.check(rc, IntervalError)


def parse_bed(text, names):
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("latin-1")
    where = {n: k for k, n in enumerate(names)}
    out = []
    for no, ln in enumerate(text.split("\n"), 1):
        f = ln.split()
        if not f or ln.startswith(("#", "track", "browser")):
            continue
        if len(f) < 3:
            raise ValueError(f"BED line {no}: fewer than three columns")
        if f[0] not in where:
            raise ValueError(f"BED line {no}: {f[0]!r} is not a contig of the table")
        try:
            out.append((where[f[0]], int(f[1]), int(f[2])))
        except ValueError:
            raise ValueError(f"BED line {no}: begin or end is not a number") from None
    return out


class Prepared(hcgenome.Prepared):
    """The arguments of a call, built once (timing tools time run() alone)."""

    def __init__(self, sam, contigs, intervals, index=None, **kw):
        super().__init__(sam, contigs, **kw)
        where = {n: k for k, n in enumerate(self.names)}

        def contig(c):
            if isinstance(c, str):
                c = c.encode("latin-1")
            if isinstance(c, bytes):
                if c not in where:
                    raise ValueError(f"interval contig {c!r} is not in the table")
                return where[c]
            return int(c)
        self.n_intervals = len(intervals)
        self.intervals = (Interval * max(self.n_intervals, 1))(*[Interval(contig(c), b, e) for c, b, e in intervals])
        self.index = None if index is None else bytes(index)

    def run(self):
        """One hc_genome_call_intervals; returns the handle (free it with free())."""
        h = C.c_void_p()
        _check(lib().hc_genome_call_intervals(self.sam, len(self.sam), self.table, self.n, self.intervals, self.n_intervals,
                                              self.region_size, self.padding_size, self.seed & (2 ** 64 - 1), self.pick,
                                              self.flags, C.byref(h)))
        return h


class PreparedBam(Prepared):
    """`sam` is the BAM file."""

    def run(self):
        """One hc_bam_genome_call_intervals."""
        h = C.c_void_p()
        _check(lib().hc_bam_genome_call_intervals(self.sam, len(self.sam), self.index, len(self.index or b""), self.table,
                                                  self.n, self.intervals, self.n_intervals, self.region_size,
                                                  self.padding_size, self.seed & (2 ** 64 - 1), self.pick, self.flags,
                                                  C.byref(h)))
        return h


def results(h, names, windows=None):
    """hcgenome.results plus ``merged`` and ``asked``."""
    out = hcgenome.results(h, names, windows)
    iv, n_iv, asked, n_asked = C.POINTER(Interval)(), C.c_int32(), _i32p(), C.c_int32()
    _check(lib().hc_genome_result_intervals(h, C.byref(iv), C.byref(n_iv), C.byref(asked), C.byref(n_asked)))
    out["merged"] = [(iv[k].contig, iv[k].begin, iv[k].end) for k in range(n_iv.value)]
    out["asked"] = asked[:n_asked.value]
    return out


def _kw(region_size, padding_size, seed, pick, skip_unplaced, use_double, want_site_reads, sorted_buckets):
    return dict(region_size=region_size, padding_size=padding_size, seed=seed, pick=pick, skip_unplaced=skip_unplaced,
                use_double=use_double, want_site_reads=want_site_reads, sorted_buckets=sorted_buckets)


def call_genome(sam, contigs, intervals, region_size=245, padding_size=85, seed=0, pick="seeded", skip_unplaced=False,
                use_double=None, want_site_reads=False, sorted_buckets=False, windows=None):
    p = Prepared(sam, contigs, intervals, **_kw(region_size, padding_size, seed, pick, skip_unplaced, use_double,
                                                want_site_reads, sorted_buckets))
    h = p.run()
    try:
        return results(h, [n.decode("latin-1") for n in p.names], windows)
    finally:
        p.free(h)


def call_genome_bam(bam, contigs, intervals, index=None, region_size=245, padding_size=85, seed=0, pick="seeded",
                    skip_unplaced=False, use_double=None, want_site_reads=False, sorted_buckets=False, windows=None):
    p = PreparedBam(bam, contigs, intervals, index, **_kw(region_size, padding_size, seed, pick, skip_unplaced, use_double,
                                                           want_site_reads, sorted_buckets))
    h = p.run()
    try:
        out = results(h, [n.decode("latin-1") for n in p.names], windows)
        out["bases"] = hcbam._bytes(hcbam.lib().hc_bam_genome_result_bases, h)
        nc, nm, up, nr = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        _check(lib().hc_bam_genome_result_index(h, C.byref(nc), C.byref(nm), C.byref(up), C.byref(nr)))
        out["index_stats"] = dict(chunks=nc.value, members=nm.value, bytes_up=up.value, records=nr.value)
        return out
    finally:
        p.free(h)
