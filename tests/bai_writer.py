"""A .bai for a coordinate-sorted BAM file made by bam_cases.to_bam, written from
the SAM specification, §5.2: records and their virtual offsets from
bam_cases.members and the block_size chain of the inflated stream, a record's
bin from reg2bin over [pos, pos + the reference length of its CIGAR), chunks of
consecutive records of one bin joined, the linear index per 16 KiB with unset
entries filled from the one before. Shared by the CPU and GPU tests of the
indexed interval call."""
from __future__ import annotations

import bisect
import struct

import bam_cases as BC

META_BIN = 37450


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reference_length(cigar_words):
    n = sum(w >> 4 for w in cigar_words if (w & 15) in (0, 2, 3, 7, 8))
    return max(n, 1)


def layout(bam):
    """(members as (coff, first inflated offset, isize), the inflated stream, [(offset, length, ref_id, pos, end)] per record)."""
    mem, at = [], 0
    for coff, _, _, isize in BC.members(bam):
        mem.append((coff, at, isize))
        at += isize
    stream = BC.inflate(bam)
    l_text, = struct.unpack_from("<i", stream, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, p)
        p += 8 + l_name
    recs = []
    while p < len(stream):
        size, rid, pos, l_name, _, _, n_cigar = struct.unpack_from("<iiiBBHH", stream, p)
        cigar = struct.unpack_from(f"<{n_cigar}I", stream, p + 36 + l_name)
        recs.append((p, 4 + size, rid, pos, pos + reference_length(cigar)))
        p += 4 + size
    return mem, stream, n_ref, recs


_cache = {}


def _firsts(mem):
    key = id(mem)
    if key not in _cache or _cache[key][0] is not mem:
        _cache.clear()
        _cache[key] = (mem, [first for _, first, _ in mem])
    return _cache[key][1]


def voffset(mem, p):
    """Of inflated offset p: the member its byte lies in; at the stream's end the last member (the EOF marker)."""
    firsts = _firsts(mem)
    k = bisect.bisect_right(firsts, p) - 1          # the last of the members that begin at or in front of p: not an empty one
    coff, first, isize = mem[k]
    if p >= first + isize:                          # the stream's end
        coff, first, _ = mem[-1]
    return coff << 16 | (p - first)


def index(bam):
    """Per reference: (bins: {bin: [(beg, end)]}, linear: [offset])."""
    mem, _, n_ref, recs = layout(bam)
    refs = [({}, []) for _ in range(n_ref)]
    last = (-1, -1)
    for at, length, rid, pos, end in recs:
        if rid < 0:
            continue
        assert (rid, pos) >= last, "the file is not coordinate-sorted"
        last = (rid, pos)
        bins, linear = refs[rid]
        beg_v, end_v = voffset(mem, at), voffset(mem, at + length)
        chunks = bins.setdefault(reg2bin(pos, end), [])
        if chunks and chunks[-1][1] == beg_v:
            chunks[-1] = (chunks[-1][0], end_v)
        else:
            chunks.append((beg_v, end_v))
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            while len(linear) <= w:
                linear.append(0)
            if linear[w] == 0:
                linear[w] = beg_v
    for _, linear in refs:
        for w in range(1, len(linear)):
            if linear[w] == 0:
                linear[w] = linear[w - 1]
    return refs


def pack(refs, meta=False, no_coor=None):
    out = [b"BAI\x01", struct.pack("<i", len(refs))]
    for bins, linear in refs:
        out.append(struct.pack("<i", len(bins) + (1 if meta else 0)))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])))
            out += [struct.pack("<QQ", *c) for c in bins[b]]
        if meta:
            out.append(struct.pack("<IiQQQQ", META_BIN, 2, 2 ** 63, 1, 7, 0))     # no chunks: beg above end, counts
        out.append(struct.pack("<i", len(linear)))
        out += [struct.pack("<Q", v) for v in linear]
    if no_coor is not None:
        out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def build(bam, meta=True, no_coor=0):
    return pack(index(bam), meta, no_coor)
