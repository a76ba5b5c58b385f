"""A plain DEFLATE walker that states what a stream exercises.

walk(stream) -> (bytes, census): the shortest possible inflater, bit by bit,
canonical codes looked up in a dictionary (length, code) -> symbol, no fast
tables, for well-formed streams only. Every test that uses a census first
asserts that the bytes are exactly zlib.decompress(stream, -15), which keeps
the walker honest.

The census (a dict; merge() is the union of several):
    blocks              the number of blocks
    block_types         the set of BTYPEs
    empty_stored        the number of stored blocks of LEN 0
    block_list          (BTYPE, bytes it gave) of every block in order
    last_block          the last entry of block_list
    lit_declared, dist_declared   the sets of code lengths a block declares (a fixed block: 7, 8, 9 and 5)
    lit_used, dist_used           the sets of code lengths of the symbols that occur
    hlit, hdist         the sets of the two fields' values (HLIT = codes - 257, HDIST = codes - 1)
    hclen               the set of the numbers of code-length code lengths sent (4...19)
    crossing_runs       the run codes (16, 17, 18) that begin in the literal/length lengths and end in
                        the distance lengths, as a list of the codes
    dist_code_counts    per dynamic block min(2, the number of distance codes), as a set
    length_symbols, dist_symbols  the sets of symbols that occur
    length_extremes, dist_extremes   (symbol, 0) where the symbol occurs with all its extra bits zero,
                        (symbol, 1) with all of them one (a symbol without extra bits counts as both)
    max_distance        the largest distance
    overlaps            the set of distances below their length
    matches             the set of (length, distance)
    matches_across_blocks   the matches that begin in front of their own block's first byte
    blocks_without_match
    ends_on_match       whether the last token in front of the last end-of-block is a match
"""
from __future__ import annotations

from deflate_writer import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA


def _table(lens):
    out, code, prev = {}, 0, 0
    for length, s in sorted((length, s) for s, length in lens.items() if length):
        code <<= length - prev
        out[length, code] = s
        code, prev = code + 1, length
    return out


def new_census():
    return dict(blocks=0, block_types=set(), empty_stored=0, last_block=None, lit_declared=set(), dist_declared=set(),
                lit_used=set(), dist_used=set(), hlit=set(), hdist=set(), hclen=set(), crossing_runs=[],
                dist_code_counts=set(), length_symbols=set(), dist_symbols=set(), length_extremes=set(),
                dist_extremes=set(), max_distance=0, overlaps=set(), matches=set(), blocks_without_match=0,
                ends_on_match=False, matches_across_blocks=0, block_list=[])


def merge(censuses):
    out = new_census()
    for c in censuses:
        for k, v in c.items():
            if isinstance(v, set):
                out[k] |= v
            elif isinstance(v, list):
                out[k] += v
            elif k in ("blocks", "empty_stored", "blocks_without_match", "matches_across_blocks"):
                out[k] += v
            elif k == "max_distance":
                out[k] = max(out[k], v)
    return out


def walk(stream: bytes):
    at = 0                       # in bits
    out = bytearray()
    c = new_census()

    def take(n):                 # n <= 16, least significant bit first
        nonlocal at
        assert at + n <= 8 * len(stream)
        v = int.from_bytes(stream[at >> 3:(at >> 3) + 3], "little") >> (at & 7) & ((1 << n) - 1)
        at += n
        return v

    def symbol(table):           # a code comes most significant bit first
        nonlocal at
        ahead = int.from_bytes(stream[at >> 3:(at >> 3) + 3], "little") >> (at & 7)
        code = 0
        for length in range(1, 16):
            code = code << 1 | (ahead >> (length - 1) & 1)
            if (length, code) in table:
                at += length
                assert at <= 8 * len(stream)
                return table[length, code], length
        raise ValueError("no such code")

    def extremes(into, s, extra, bits):
        if extra == 0:
            into.add((s, 0))
        if extra == (1 << bits) - 1:
            into.add((s, 1))

    while True:
        last, kind = take(1), take(2)
        c["blocks"] += 1
        c["block_types"].add(kind)
        before = len(out)
        if kind == 0:
            at = (at + 7) & ~7
            n, inv = take(16), take(16)
            assert n ^ inv == 0xFFFF
            out += stream[at >> 3:(at >> 3) + n]
            assert len(out) - before == n
            at += 8 * n
            c["empty_stored"] += n == 0
            c["blocks_without_match"] += 1
            c["ends_on_match"] = False
        else:
            assert kind in (1, 2)
            if kind == 1:
                lit_lens, dist_lens = dict(FIXED_LIT), dict(FIXED_DIST)
            else:
                nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
                c["hlit"].add(nlen - 257)
                c["hdist"].add(ndist - 1)
                c["hclen"].add(ncode)
                cl = _table({CL_ORDER[k]: take(3) for k in range(ncode)})
                lens = []
                while len(lens) < nlen + ndist:
                    s, _ = symbol(cl)
                    if s < 16:
                        lens.append(s)
                        continue
                    rep = 3 + take(2) if s == 16 else 3 + take(3) if s == 17 else 11 + take(7)
                    if len(lens) < nlen < len(lens) + rep:
                        c["crossing_runs"].append(s)
                    lens += [lens[-1] if s == 16 else 0] * rep
                assert len(lens) == nlen + ndist
                lit_lens, dist_lens = dict(enumerate(lens[:nlen])), dict(enumerate(lens[nlen:]))
                c["dist_code_counts"].add(min(2, sum(1 for v in dist_lens.values() if v)))
            c["lit_declared"] |= {v for v in lit_lens.values() if v}
            c["dist_declared"] |= {v for v in dist_lens.values() if v}
            lit, dist = _table(lit_lens), _table(dist_lens)
            matched = False
            while True:
                s, length = symbol(lit)
                c["lit_used"].add(length)
                if s < 256:
                    out.append(s)
                    c["ends_on_match"] = False
                    continue
                if s == 256:
                    break
                assert s <= 285
                bits = LEN_EXTRA[s - 257]
                extra = take(bits)
                n = LEN_BASE[s - 257] + extra
                c["length_symbols"].add(s)
                extremes(c["length_extremes"], s, extra, bits)
                d, length = symbol(dist)
                assert d <= 29
                c["dist_used"].add(length)
                bits = DIST_EXTRA[d]
                extra = take(bits)
                back = DIST_BASE[d] + extra
                c["dist_symbols"].add(d)
                extremes(c["dist_extremes"], d, extra, bits)
                assert back <= len(out)
                for _ in range(n):
                    out.append(out[-back])
                c["max_distance"] = max(c["max_distance"], back)
                c["matches"].add((n, back))
                c["matches_across_blocks"] += back > len(out) - n - before
                if back < n:
                    c["overlaps"].add(back)
                matched = True
                c["ends_on_match"] = True
            c["blocks_without_match"] += not matched
        c["block_list"].append((kind, len(out) - before))
        if last:
            c["last_block"] = (kind, len(out) - before)
            return bytes(out), c
