"""A DEFLATE writer that does what it is told, for the inputs of the BGZF
inflater's tests (bam_cases.written_cases() and its malformed twins). Built on
bam_cases.Bits, standard library only.

Tokens: an int is a literal; (length, distance) is a match, its length written
with the symbol of RFC 1951's table; (length, distance, symbol) names the length
symbol, which matters for length 258 alone: symbol 285, or symbol 284 with its
five extra bits all one.

    expand(tokens)                       the bytes the tokens stand for
    stored(bits, raw, last)              a stored block
    fixed(bits, tokens, last)            a fixed block
    dynamic(bits, tokens, lit_lens, dist_lens, last, nlen=None, ndist=None)
                                         a dynamic block with the given code lengths
                                         (dicts symbol -> length)
    complete(n, max_len)                 n code lengths with Kraft sum exactly 1

The header of dynamic() is run-length coded over the concatenated array of
nlen + ndist lengths (greedily: 18, then 17 for zeros, 16 for repeats), so a run
crosses from the literal/length lengths into the distance lengths wherever the
values allow; its code-length code is complete(., 7) over the code-length
symbols it uses, the shortest codes on the most frequent; HCLEN is as small as
the order allows. The pieces (run_lengths, header, body, canonical) are public
so that a malformed case can write the part it breaks by hand.

The writer never chooses on its own: what it emits is what the case asked for.
A symbol without a code length is a KeyError, not a quiet fallback.
"""
from __future__ import annotations

from bam_cases import Bits

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = {s: 8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8 for s in range(288)}
FIXED_DIST = {s: 5 for s in range(32)}


def length_symbol(length: int) -> int:
    """The symbol (257...285) RFC 1951's table gives a length; 258 is symbol 285."""
    assert 3 <= length <= 258
    return 257 + max(k for k in range(29) if LEN_BASE[k] <= length)


def distance_symbol(dist: int) -> int:
    assert 1 <= dist <= 32768
    return max(k for k in range(30) if DIST_BASE[k] <= dist)


def expand(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out), (dist, len(out))
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def symbols_of(tokens):
    """(literal/length symbols, distance symbols) of the tokens with their counts, end-of-block included."""
    lit, dist = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lit[t] = lit.get(t, 0) + 1
        else:
            s = t[2] if len(t) > 2 else length_symbol(t[0])
            lit[s] = lit.get(s, 0) + 1
            d = distance_symbol(t[1])
            dist[d] = dist.get(d, 0) + 1
    return lit, dist


def complete(n: int, max_len: int):
    """n code lengths, ascending, with Kraft sum exactly 1, as deep as max_len allows: from (1, 1), the deepest
    code below max_len is split into two again and again. n = 1 gives the one code of one bit (Kraft sum 1/2)."""
    assert 1 <= n <= 1 << max_len
    if n == 1:
        return [1]
    lens = [1, 1]
    while len(lens) < n:
        k = max((k for k in range(len(lens)) if lens[k] < max_len), key=lambda k: (lens[k], k))
        lens[k:k + 1] = [lens[k] + 1, lens[k] + 1]
        lens.sort()
    return lens


def canonical(lens):
    """symbol -> (code, length) of the canonical Huffman code of a dict symbol -> length (0: no code)."""
    out, code, prev = {}, 0, 0
    for length, s in sorted((length, s) for s, length in lens.items() if length):
        code <<= length - prev
        out[s] = (code, length)
        code, prev = code + 1, length
    return out


def stored(bits: Bits, raw: bytes, last: bool, nlen_xor=0xFFFF):
    bits.put(int(last), 1).put(0, 2)
    bits.put(0, -bits.n % 8)
    bits.put(len(raw), 16).put(len(raw) ^ nlen_xor, 16)
    for c in raw:
        bits.put(c, 8)
    return bits


def body(bits: Bits, tokens, lit_codes, dist_codes, end=True):
    for t in tokens:
        if isinstance(t, int):
            bits.code(*lit_codes[t])
            continue
        length, dist = t[0], t[1]
        s = t[2] if len(t) > 2 else length_symbol(length)
        assert 0 <= length - LEN_BASE[s - 257] < 1 << LEN_EXTRA[s - 257] or length == LEN_BASE[s - 257], t
        bits.code(*lit_codes[s])
        bits.put(length - LEN_BASE[s - 257], LEN_EXTRA[s - 257])
        d = distance_symbol(dist)
        bits.code(*dist_codes[d])
        bits.put(dist - DIST_BASE[d], DIST_EXTRA[d])
    if end:
        bits.code(*lit_codes[256])
    return bits


def fixed(bits: Bits, tokens, last: bool):
    bits.put(int(last), 1).put(1, 2)
    return body(bits, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def run_lengths(lens):
    """The code-length symbols [(symbol, extra bits' value)] of a length array, greedily."""
    out, k = [], 0
    while k < len(lens):
        v, run = lens[k], 1
        while k + run < len(lens) and lens[k + run] == v:
            run += 1
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18, take - 11) if take >= 11 else (17, take - 3))
            k += take
            continue
        out.append((v, 0))
        k += 1
        run -= 1
        while run >= 3:
            take = min(run, 6)
            out.append((16, take - 3))
            k += take
            run -= take
    return out


def header(bits: Bits, last: bool, hlit: int, hdist: int, cl_lens, cl_tokens, hclen=None):
    """BFINAL, BTYPE 2, the three counts as their fields' values, the code-length code's lengths in their
    order and the code-length symbols, all as given."""
    if hclen is None:
        hclen = max([4] + [k + 1 for k in range(19) if cl_lens.get(CL_ORDER[k], 0)])
    bits.put(int(last), 1).put(2, 2).put(hlit, 5).put(hdist, 5).put(hclen - 4, 4)
    for k in range(hclen):
        bits.put(cl_lens.get(CL_ORDER[k], 0), 3)
    codes = canonical(cl_lens)
    for s, extra in cl_tokens:
        bits.code(*codes[s])
        bits.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
    return bits


def code_length_code(cl_tokens):
    """symbol -> length: complete(., 7) over the symbols in use, the shortest codes on the most frequent. A
    code-length code must be complete, so a lone symbol gets an unused partner."""
    count = {}
    for s, _ in cl_tokens:
        count[s] = count.get(s, 0) + 1
    if len(count) == 1:
        count[0 if 0 not in count else 1] = 0
    order = sorted(count, key=lambda s: (-count[s], s))
    return dict(zip(order, complete(len(order), 7)))


def dynamic_header(bits: Bits, lit_lens, dist_lens, last: bool, nlen=None, ndist=None):
    nlen = max([257] + [s + 1 for s, v in lit_lens.items() if v]) if nlen is None else nlen
    ndist = max([1] + [s + 1 for s, v in dist_lens.items() if v]) if ndist is None else ndist
    lens = [lit_lens.get(s, 0) for s in range(nlen)] + [dist_lens.get(s, 0) for s in range(ndist)]
    cl_tokens = run_lengths(lens)
    return header(bits, last, nlen - 257, ndist - 1, code_length_code(cl_tokens), cl_tokens)


def dynamic(bits: Bits, tokens, lit_lens, dist_lens, last: bool, nlen=None, ndist=None):
    dynamic_header(bits, lit_lens, dist_lens, last, nlen, ndist)
    return body(bits, tokens, canonical(lit_lens), canonical(dist_lens))


def lens_by_use(count, max_len=15):
    """A case's choice, not the writer's: complete(., max_len) over the symbols of `count`, the shortest codes on
    the most used."""
    order = sorted(count, key=lambda s: (-count[s], s))
    return dict(zip(order, complete(len(order), max_len))) if order else {}
