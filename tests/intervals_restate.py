"""The rules of an interval call (include/hc_intervals.h) restated in Python,
without a binary search and without the arithmetic of interval_body.hpp: sets
of positions and loops over every window. Shared by test_intervals_host.py (the
host program under the sanitizers) and the GPU tests of the interval calls.

An interval is (contig index, begin, end), 0-based and half-open.
"""
from __future__ import annotations


def check(intervals, ref_lens):
    """The index of the first interval that is no range of its contig, or None."""
    for k, (c, b, e) in enumerate(intervals):
        if not 0 <= c < len(ref_lens) or b < 0 or e <= b or e > ref_lens[c]:
            return k
    return None


def merge(intervals):
    """Sorted by contig, then begin; overlapping, abutting and duplicate intervals joined: the maximal runs of covered
    positions."""
    out = []
    for c in sorted({c for c, _, _ in intervals}):
        covered = set()
        for cc, b, e in intervals:
            if cc == c:
                covered.update(range(b, e))
        run = None
        for p in sorted(covered):
            if run is not None and p == run[1]:
                run[1] = p + 1
            else:
                if run is not None:
                    out.append((c, run[0], run[1]))
                run = [p, p + 1]
        out.append((c, run[0], run[1]))
    return out


def merge_sorted(intervals):
    """merge() for long intervals: by sorting, not by sets of positions."""
    out = []
    for c, b, e in sorted(intervals):
        if out and out[-1][0] == c and b <= out[-1][2]:
            out[-1][2] = max(out[-1][2], e)
        else:
            out.append([c, b, e])
    return [tuple(x) for x in out]


def windows(ref_len, region, padding):
    """Per window of a contig: (padded_begin, padded_end, origin_begin, origin_end), origin_end cut at the contig's end."""
    out = []
    for lw in range(-(-ref_len // region)):
        ob = lw * region
        out.append((0 if lw == 0 else ob - padding, ob + region + padding, ob, min(ob + region, ref_len)))
    return out


def asked(intervals, ref_lens, region, padding):
    """The genome-wide windows whose own bases meet an interval, ascending."""
    out, first = [], 0
    for c, n in enumerate(ref_lens):
        mine = [(b, e) for cc, b, e in intervals if cc == c]
        ws = windows(n, region, padding)
        out += [first + lw for lw, (_, _, ob, oe) in enumerate(ws) if any(b < oe and ob < e for b, e in mine)]
        first += len(ws)
    return out


def windows_of(p, ref_len, region, padding):
    """The windows of the contig whose padded interval holds position p."""
    return [lw for lw, (pb, pe, _, _) in enumerate(windows(ref_len, region, padding)) if pb <= p < pe]


def in_scope(c, pos, ref_lens, region, padding, asked_windows):
    """A record of contig c (-1: none) with 1-based POS: placed, and a window that holds POS - 1 is asked."""
    if c < 0 or pos == 0 or pos - 1 >= ref_lens[c]:
        return False
    first = sum(len(windows(n, region, padding)) for n in ref_lens[:c])
    return any(first + lw in asked_windows for lw in windows_of(pos - 1, ref_lens[c], region, padding))


def inside(intervals, c, p):
    """Position p of contig c lies inside an interval."""
    return any(cc == c and b <= p < e for cc, b, e in intervals)


# ---- the BAM index (SAM specification §5.2), restated without the shifts of reg2bins ----------

LEVELS = ((0, 29), (1, 26), (9, 23), (73, 20), (585, 17), (4681, 14))   # (a level's first bin, log2 of a bin's span)
META_BIN = 37450


def parse_bai(data):
    """[(bins: {bin: [(beg, end)]}, linear)] per reference; the metadata pseudo-bin left out."""
    import struct
    assert data[:4] == b"BAI\x01"
    n_ref, = struct.unpack_from("<i", data, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", data, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b != META_BIN:
                bins[b] = chunks
        n_intv, = struct.unpack_from("<i", data, at)
        at += 4
        refs.append((bins, list(struct.unpack_from(f"<{n_intv}Q", data, at))))
        at += 8 * n_intv
    return refs


def bins_of(beg, end):
    """Every bin whose span meets [beg, end)."""
    out = []
    for first, log2 in LEVELS:
        span = 1 << log2
        out += [first + k for k in range(1 << (29 - log2)) if k * span < end and beg < (k + 1) * span] if log2 >= 20 else \
               [first + k for k in range(beg // span, (end - 1) // span + 1)]
    return out


def query(refs, ref, beg, end):
    """The chunks of the candidate bins, but those that end at or in front of the linear offset of beg's 16 KiB window."""
    bins, linear = refs[ref]
    floor = linear[min(beg // 16384, len(linear) - 1)] if linear else 0
    return [c for b in bins_of(beg, end) for c in bins.get(b, []) if c[1] > floor]


def merge_chunks(chunks):
    out = []
    for beg, end in sorted(chunks):
        if out and (beg <= out[-1][1] or beg >> 16 <= out[-1][1] >> 16):
            out[-1][1] = max(out[-1][1], end)
        else:
            out.append([beg, end])
    return [tuple(c) for c in out]


def ranges(intervals, ref_lens, region, padding):
    """Per run of consecutive asked windows of a contig: (contig, first.padded_begin, min(last.padded_end, ref_len))."""
    out, first = [], 0
    is_asked = set(asked(intervals, ref_lens, region, padding))
    for c, n in enumerate(ref_lens):
        ws = windows(n, region, padding)
        run = None
        for lw in range(len(ws) + 1):
            if lw < len(ws) and first + lw in is_asked:
                run = [lw, lw] if run is None else [run[0], lw]
            elif run is not None:
                out.append((c, ws[run[0]][0], min(ws[run[1]][1], n)))
                run = None
        first += len(ws)
    return out


def members_read(chunks, member_coffs):
    """The members from each merged chunk's first to the one its end lands in (not that one when the in-member offset is 0)."""
    got = set()
    for beg, end in chunks:
        got |= {c for c in member_coffs if beg >> 16 <= c and (c < end >> 16 or (c == end >> 16 and end & 0xffff))}
    return sorted(got)


def chosen_members(bai, intervals, ref_lens, ref_of, region, padding, member_coffs):
    """What the specification's query reads for the interval list: ref_of[c] is contig c's refID."""
    refs = parse_bai(bai)
    chunks = []
    for c, beg, end in ranges(merge_sorted(intervals), ref_lens, region, padding):
        chunks += query(refs, ref_of[c], beg, end)
    return members_read(merge_chunks(chunks), member_coffs)
