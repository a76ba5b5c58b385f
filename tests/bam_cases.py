"""BGZF and BAM inputs shared by the tests of the BAM front (test_bgzf_host.py,
test_gpu_bgzf.py, test_gpu_bam.py, test_gpu_bam_genome.py) and tools/bam_timing.py.
Standard library only (zlib, struct): the files are written here, byte by byte.

to_bam(sam_text, refs, member_size, level, strategy, mem_level): the records of
a SAM text as a BAM file in real BGZF, every member one
zlib.compressobj(level, DEFLATED, -15, mem_level, strategy) stream with its
CRC32, ISIZE and BSIZE, and the empty end-of-file member.
sam_of(bam): the text `samtools view -h` prints for it, without auxiliary tags
(the canonical text T of include/hc_bam.h), inflated with zlib.decompress.

bgzf_cases(): well-formed BGZF files by name with their inflated bytes;
malformed_cases(): (file, the 0-based member the error names, its BgzfError code).
A member's whole size is at most 65 536 bytes (BSIZE has 16 bits), so a stored
block of 65 535 bytes cannot stand in a BGZF member: the largest stored block
here has 65 000 bytes, with a second block behind it in the same member.
Every stream of bgzf_cases() is zlib's, and zlib uses a narrow part of the
format: in these files no code longer than 12 bits, always two distance codes
at least, the two alphabets' lengths coded apart, no distance above 32 503
(zlib's window stops 262 bytes short of 32 768, so second_half_repeats, whose
second half repeats the first 32 768 bytes back, is not copied at that distance).

What zlib never writes (what each input exercises is asserted from a census of
its streams in test_bgzf_census.py):
written_cases(): name -> (raw DEFLATE stream, bytes) from deflate_writer:
    deep15                     code lengths 1...15, 15 in both alphabets, the 15-bit codes on end-of-block,
                               symbol 285 and distance symbols 28 and 29, HCLEN 19, a last match of 258 at
                               distance 32 768
    every_code_fixed / _dynamic   all 29 length and 30 distance symbols with their extra bits all zero and all one
                               (258 as symbol 284 + 31 too), distance 32 768; _dynamic under HLIT = HDIST = 29
    overlaps                   distances 1...66, 127, 128, 129, 257, each with lengths 3, 64, 65, 258
    no_distance_code, one_distance_code, hlit_0
    run_across_alphabets, zero_run_across_alphabets   a run code 16 / 18 from the literal/length lengths into
                               the distance lengths
    tiny_blocks                1 504 blocks: fixed, dynamic, stored, empty stored in turn, matches across their
                               borders, the last an empty stored block
    ends_on_a_match            ISIZE 65 536, the last token a match of 258
    stored_then_far_match      a match at distance 20 000 to the member's first byte, through a stored block
written_file(): (file, bytes), every case a member, three of them again behind members of odd sizes.
alignment_file(): (file, bytes), 118 small zlib members, every out_off & 15 against ISIZE 1, 2, 15, 16, 17, 31, 33.
written_malformed_cases(): as malformed_cases(), the DEFLATE errors that one is without.
libdeflate_members(): the streams of tests/golden/libdeflate_members.npz, a second producer's.
mutants(n, seed): seeded edits of small streams with zlib's verdict (zlib_verdict) as the expected one.
bgzf(..., compress=) / to_bam(..., compress=): members from another writer, e.g. written_compress.
"""
from __future__ import annotations

import functools
import os
import random
import struct
import zlib

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
SPACE = " \t\v\f\r"
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# hcbgzf::BgzfError
ERR_HEADER, ERR_BSIZE, ERR_ISIZE, ERR_STREAM, ERR_EARLY, ERR_COUNT, ERR_DISTANCE, ERR_CRC = range(1, 9)


# ---- BGZF ------------------------------------------------------------------------------

def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_at=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def member(stream: bytes, crc: int, isize: int, bsize=None, magic=b"\x1f\x8b") -> bytes:
    """One BGZF member around a raw DEFLATE stream; crc, isize and bsize are written as given."""
    total = 18 + len(stream) + 8
    assert total <= 65536, total
    head = magic + b"\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, (
        total if bsize is None else bsize) - 1)
    return head + stream + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def good_member(data: bytes, **kw) -> bytes:
    return member(deflate(data, **kw), zlib.crc32(data), len(data))


def bgzf(data: bytes, member_size=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, eof=True,
         compress=None) -> bytes:
    """compress: bytes -> a raw DEFLATE stream, in place of zlib's."""
    if compress is None:
        def compress(piece):
            return deflate(piece, level=level, strategy=strategy, mem_level=mem_level)
    out = b"".join(member(compress(data[k:k + member_size]), zlib.crc32(data[k:k + member_size]),
                          len(data[k:k + member_size])) for k in range(0, len(data), member_size))
    return out + (EOF_MARKER if eof else b"")


def members(file: bytes):
    """[(coff, stream, crc, isize)] of a well-formed BGZF file."""
    out, off = [], 0
    while off < len(file):
        assert file[off:off + 4] == b"\x1f\x8b\x08\x04"
        xlen, = struct.unpack_from("<H", file, off + 10)
        assert file[off + 12:off + 16] == b"BC\x02\x00"
        total = struct.unpack_from("<H", file, off + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", file, off + total - 8)
        out.append((off, file[off + 12 + xlen:off + total - 8], crc, isize))
        off += total
    return out


def inflate(file: bytes) -> bytes:
    out = []
    for _, stream, crc, isize in members(file):
        data = zlib.decompress(stream, -15)
        assert len(data) == isize and zlib.crc32(data) == crc
        out.append(data)
    return b"".join(out)


def first_block_type(stream: bytes) -> int:
    """BTYPE of a DEFLATE stream's first block: 0 stored, 1 fixed, 2 dynamic."""
    return (stream[0] >> 1) & 3


class Bits:
    """A DEFLATE bit writer: put() least significant bit first, code() a Huffman code, most significant first.
    n is the number of bits written so far."""

    def __init__(self):
        self.buf, self.acc, self.k = bytearray(), 0, 0

    @property
    def n(self):
        return 8 * len(self.buf) + self.k

    def put(self, value, n):
        self.acc |= value << self.k
        self.k += n
        if self.k >= 8:
            whole = self.k >> 3
            self.buf += (self.acc & ((1 << 8 * whole) - 1)).to_bytes(whole, "little")
            self.acc >>= 8 * whole
            self.k &= 7
        return self

    def code(self, code, n):
        return self.put(int(format(code, f"0{n}b")[::-1], 2), n) if n else self

    def bytes(self):
        return bytes(self.buf) + (bytes([self.acc & 255]) if self.k else b"")


def _rng_bytes(seed, n, alphabet=None):
    r = random.Random(seed)
    if alphabet is None:
        return r.randbytes(n)
    return bytes(r.choices(alphabet, k=n))


def _texty(seed, n):
    """Compressible, not trivially: words over a small alphabet with repeats at many distances."""
    r = random.Random(seed)
    words = [bytes(r.choices(b"ACGTNacgt\t\n0123456789", k=r.randint(2, 40))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words)
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def bgzf_cases():
    """name -> (file, inflated bytes)."""
    text = _texty(1, 200000)
    out = {}

    def add(name, file):
        out[name] = (file, inflate(file))
    add("eof_only", EOF_MARKER)
    add("isize_0_then_data", good_member(b"") + good_member(b"x" * 10) + EOF_MARKER)
    add("isize_1", bgzf(b"A"))
    add("isize_65280", bgzf(text[:65280]))
    add("isize_65536", bgzf(text[:65536], member_size=65536))
    add("level_0", bgzf(text[:70000], level=0))
    # a stored block of 65 000 bytes that is not the last, then a second block, in one member
    tail = text[:500]
    stored = b"\x00" + struct.pack("<HH", 65000, 65000 ^ 0xFFFF) + _rng_bytes(2, 65000)
    two = stored[5:] + tail
    add("stored_then_dynamic", member(stored + deflate(tail, level=9), zlib.crc32(two), len(two)) + EOF_MARKER)
    add("fixed", bgzf(text[:150000], strategy=zlib.Z_FIXED))
    add("level_1", bgzf(text, level=1))
    add("level_6", bgzf(text, level=6))
    add("level_9", bgzf(text, level=9))
    add("mem_level_1", bgzf(text[:131000], mem_level=1, member_size=65500))
    add("full_flush", good_member(text[:50000], flush_at=20000) + EOF_MARKER)
    add("one_byte_run", bgzf(b"z" * 65536, member_size=65536))
    half = _rng_bytes(3, 32768, b"ACGT")
    add("second_half_repeats", bgzf(half + half, member_size=65536, level=9))
    add("random", bgzf(_rng_bytes(4, 130000), member_size=65000))
    add("no_eof_marker", bgzf(text[:100000], eof=False))
    r = random.Random(5)
    mixed = []
    for k in range(300):
        n = r.choice([0, 1, 2, 17, 300, 5000, 20000, 60000])
        data = (_texty(100 + k, n), _rng_bytes(100 + k, n), b"ab" * (n // 2) + b"a" * (n % 2))[k % 3]
        kind = k % 5
        mixed.append(good_member(data, level=(0, 1, 6, 9, 6)[kind],
                                 strategy=zlib.Z_FIXED if kind == 4 and k % 3 != 1 else zlib.Z_DEFAULT_STRATEGY,
                                 mem_level=1 if k % 7 == 0 else 8))
    add("mixed_300", b"".join(mixed) + EOF_MARKER)
    return out


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """name -> (file, the 0-based member the message names, the BgzfError code)."""
    text = _texty(7, 90000)
    parts = [text[:30000], text[30000:60000], text[60000:]]
    good = [good_member(p) for p in parts]
    streams = [deflate(p) for p in parts]
    crcs = [zlib.crc32(p) for p in parts]

    def with_second(m, at=1):
        g = list(good)
        g[at] = m
        return b"".join(g) + EOF_MARKER
    over = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4)
    for _ in range(4):
        over.put(1, 3)                       # four code-length codes of one bit each
    over.put(0, 32)
    # fixed block: the literal 'a' (code 0x30 + 97, 8 bits), then length 3 (symbol 257: 0000001) at distance 2 (code 1)
    before = Bits().put(1, 1).put(1, 2).code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7)
    out = dict(
        crc_flipped=(with_second(member(streams[1], crcs[1] ^ 0x10, 30000)), 1, ERR_CRC),
        isize_plus_one=(with_second(member(streams[1], crcs[1], 30001)), 1, ERR_COUNT),
        isize_minus_one=(with_second(member(streams[1], crcs[1], 29999)), 1, ERR_COUNT),
        stream_cut=(with_second(member(streams[1][:len(streams[1]) // 2], crcs[1], 30000)), 1, ERR_EARLY),
        bsize_past_end=((good[0] + good[1] + good[2])[:-100], 2, ERR_BSIZE),
        oversubscribed=(with_second(member(over.bytes(), 0, 10)), 1, ERR_STREAM),
        distance_before_start=(with_second(member(before.bytes(), 0, 4)), 1, ERR_DISTANCE),
        wrong_magic=(with_second(b"\x1f\x8c" + good[1][2:]), 1, ERR_HEADER),
        no_bc_subfield=(with_second(good[1][:12] + b"XY" + good[1][14:]), 1, ERR_HEADER),
        isize_too_large=(with_second(member(streams[1], crcs[1], 65537)), 1, ERR_ISIZE),
        two_bad=(good[0] + member(streams[1], crcs[1] ^ 1, 30000) + member(streams[2], crcs[2] ^ 1, 30000) + EOF_MARKER,
                 1, ERR_CRC),
        first_bad=(member(streams[0], crcs[0] ^ 1, 30000) + good[1] + EOF_MARKER, 0, ERR_CRC),
    )
    return out


def malformed_offset(member_index: int) -> int:
    """Where member `member_index` of a malformed file begins: the members in front of the bad one are the good ones."""
    text = _texty(7, 90000)
    return sum(len(good_member(text[k * 30000:(k + 1) * 30000])) for k in range(member_index))


# ---- streams that zlib never writes ---------------------------------------------------------

def zlib_verdict(stream: bytes):
    """What zlib makes of a raw DEFLATE stream as a BGZF member's: its bytes when decompressobj(-15) reaches the
    end of the last block with at most 65 536 bytes, None when it refuses or the stream ends early."""
    d = zlib.decompressobj(-15)
    try:
        data = d.decompress(stream, 65537)
    except zlib.error:
        return None
    return data if d.eof and len(data) <= 65536 else None


def zlib_overflows(stream: bytes) -> bool:
    """Whether zlib, fed a byte at a time, has given more than 65 536 bytes when the stream ends or zlib refuses
    it: the one way in which a member of ISIZE 65 536 with a stream that zlib refuses may end with ERR_COUNT."""
    d, n = zlib.decompressobj(-15), 0
    try:
        for k in range(len(stream)):
            n += len(d.decompress(stream[k:k + 1]))
            if n > 65536:
                return True
    except zlib.error:
        pass
    return False


def lz_tokens(data: bytes):
    """Tokens of deflate_writer for data: a greedy matcher on the last place of every three bytes."""
    toks, last, k, n = [], {}, 0, len(data)
    while k < n:
        key = data[k:k + 3]
        cand = last.get(key) if len(key) == 3 else None
        length = 0
        if cand is not None and k - cand <= 32768:
            while length < 258 and k + length < n and data[cand + length] == data[k + length]:
                length += 1
        if length >= 3:
            toks.append((length, k - cand))
            last[key] = k
            k += length
        else:
            last[key] = k
            toks.append(data[k])
            k += 1
    return toks


def written_compress(data: bytes) -> bytes:
    """data as one dynamic block from the writer: complete(., 15) lengths over the symbols lz_tokens(data) uses,
    the shortest codes on the most used."""
    import deflate_writer as W
    toks = lz_tokens(data)
    lit, dist = W.symbols_of(toks)
    return W.dynamic(Bits(), toks, W.lens_by_use(lit), W.lens_by_use(dist), True).bytes()


def _deep15_lens():
    lit = {c: k + 1 for k, c in enumerate(b"ACGTNacgtn\t\n01")}
    lit[256] = lit[285] = 15
    dist = {14 + k: k + 1 for k in range(14)}
    dist[28] = dist[29] = 15
    return lit, dist


def _every_code_tokens():
    import deflate_writer as W
    r = random.Random(13)
    toks, pos = list(range(256)), 256
    while pos < 32768:
        toks.append((258, r.choice((256, 255, 131, 64, 7))))
        pos += 258
    lengths = [(W.LEN_BASE[k] + hi * ((1 << W.LEN_EXTRA[k]) - 1), 257 + k) for k in range(29) for hi in (0, 1)]
    dists = [W.DIST_BASE[d] + hi * ((1 << W.DIST_EXTRA[d]) - 1) for d in range(30) for hi in (0, 1)]
    for i, dist in enumerate(dists):
        length, s = lengths[i % len(lengths)]
        toks += [(length, dist, s), r.randrange(256)]
    return toks


@functools.lru_cache(maxsize=None)
def written_cases():
    """name -> (raw DEFLATE stream, its bytes), every stream from deflate_writer; see the module's docstring of
    test_bgzf_census.py for the property each one carries."""
    import deflate_writer as W
    out = {}

    def add(name, bits, toks):
        out[name] = (bits.bytes(), W.expand(toks))

    # deep15
    r = random.Random(11)
    lit_lens, dist_lens = _deep15_lens()
    lits = [c for c in lit_lens if c < 256]
    toks, pos = list(lits), len(lits)

    def far(d):
        return W.DIST_BASE[d] + r.randrange(1 << W.DIST_EXTRA[d])
    while pos < 33000:
        toks += r.choices(lits, weights=[2.0 ** -k for k in range(len(lits))], k=40)
        pos += 40
        dist = far(r.randrange(14, 30))
        if dist <= pos and r.random() < 0.3:
            toks.append((258, dist))
            pos += 258
    for d in range(14, 30):
        toks += [(258, far(d)), r.choice(lits)]
    pos = len(W.expand(toks))
    assert pos >= 32768
    toks.append((258, 32768))
    add("deep15", W.dynamic(Bits(), toks, lit_lens, dist_lens, True), toks)

    # every_code_*
    toks = _every_code_tokens()
    add("every_code_fixed", W.fixed(Bits(), toks, True), toks)
    add("every_code_dynamic", W.dynamic(Bits(), toks, dict(zip(range(286), W.complete(286, 15))),
                                        dict(zip(range(30), W.complete(30, 15))), True), toks)

    # overlaps
    r = random.Random(14)
    toks = list(r.randbytes(300))
    for dist in list(range(1, 67)) + [127, 128, 129, 257]:
        for length in (3, 64, 65, 258):
            toks += [(length, dist), r.randrange(256), r.randrange(256)]
    add("overlaps", W.fixed(Bits(), toks, True), toks)

    # no_distance_code: HDIST = 0 and that one length 0
    toks = list(_texty(15, 701))
    add("no_distance_code", W.dynamic(Bits(), toks, W.lens_by_use(W.symbols_of(toks)[0]), {}, True, ndist=1), toks)

    # one_distance_code: distance symbol 9 (25...32) with one bit
    r = random.Random(16)
    toks = list(r.randbytes(45))
    for length in (3, 258, 10, 64, 31, 32, 33, 4, 258, 200):
        toks += [(length, 25 + r.randrange(8)), r.randrange(256)]
    add("one_distance_code", W.dynamic(Bits(), toks, W.lens_by_use(W.symbols_of(toks)[0]), {9: 1}, True), toks)

    # run_across_alphabets: ... 257, 258, 259 | 0, 1, 2 ... all of three bits
    r = random.Random(17)
    toks = list(b"abcdabdcbadcdcba")
    for _ in range(60):
        toks += [r.choice(b"abcd"), (r.choice((3, 4, 5)), r.randrange(1, 17))]
    add("run_across_alphabets", W.dynamic(Bits(), toks, {s: 3 for s in (97, 98, 99, 100, 256, 257, 258, 259)},
                                          {d: 3 for d in range(8)}, True), toks)

    # zero_run_across_alphabets: zeros from 258 to 269 and on distance symbols 0 to 9
    toks = list(b"ab" * 20 + b"ba" * 15)
    for _ in range(30):
        toks += [r.choice(b"ab"), (3, r.randrange(33, 65))]
    add("zero_run_across_alphabets", W.dynamic(Bits(), toks, {97: 2, 98: 2, 256: 2, 257: 2}, {10: 1, 11: 1}, True, nlen=270),
        toks)

    # hlit_0
    toks = list(_texty(18, 333))
    add("hlit_0", W.dynamic(Bits(), toks, W.lens_by_use(W.symbols_of(toks)[0]), {0: 1, 1: 1}, True), toks)

    # tiny_blocks: fixed, dynamic, stored, empty stored, 376 times
    r = random.Random(19)
    bits, whole = Bits(), []
    for i in range(376):
        pos = len(whole) if i < 3 else 99            # enough behind for every distance below
        toks = ([(3 + i % 5, 4 + i % 9)] if pos > 12 else []) + [r.randrange(256), r.randrange(256)]
        W.fixed(bits, toks, False)
        whole += toks
        toks = [(3 + i % 4, 2 + i % 3), r.randrange(256), (5, 1 + i % 7)]
        lit, dist = W.symbols_of(toks)
        W.dynamic(bits, toks, W.lens_by_use(lit), W.lens_by_use(dist), False)
        whole += toks
        raw = r.randbytes(3)
        W.stored(bits, raw, False)
        whole += list(raw)
        W.stored(bits, b"", i == 375)
    add("tiny_blocks", bits, whole)

    # ends_on_a_match
    r = random.Random(20)
    toks = list(_texty(21, 2000))
    pos = 2000
    while pos + 259 <= 65536 - 258:
        toks += [(258, r.randrange(1, min(pos, 32768) + 1)), r.randrange(256)]
        pos += 259
    toks += list(r.randbytes(65536 - 258 - pos)) + [(258, 1000)]
    lit, dist = W.symbols_of(toks)
    add("ends_on_a_match", W.dynamic(Bits(), toks, W.lens_by_use(lit), W.lens_by_use(dist), True), toks)

    # a match that reaches the member's first byte from deep inside, through a stored block
    raw = _rng_bytes(22, 20000)
    toks = [(258, 20000), 120]
    add("stored_then_far_match", W.fixed(W.stored(Bits(), raw, False), toks, True), list(raw) + toks)
    return out


def file_of(streams_and_bytes, eof=True):
    """(file, bytes) of [(raw DEFLATE stream, its bytes)]: a member each, then the end-of-file member."""
    pairs = list(streams_and_bytes)
    file = b"".join(member(s, zlib.crc32(d), len(d)) for s, d in pairs) + (EOF_MARKER if eof else b"")
    return file, b"".join(d for _, d in pairs)


AGAIN = ("deep15", "overlaps", "one_distance_code")


def written_names():
    """The case of every member of written_file() but the last."""
    return list(written_cases()) + list(AGAIN)


@functools.lru_cache(maxsize=None)
def written_file():
    """(file, bytes): every case of written_cases() as a member, then AGAIN behind members of odd sizes."""
    c = written_cases()
    return file_of(c[name] for name in written_names())


ALIGN_CLASSES = (1, 2, 15, 16, 17, 31, 33)
ALIGN_STEPS = (63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def alignment_file():
    """(file, bytes): small zlib members such that every out_off & 15 meets every ISIZE of ALIGN_CLASSES. Pairs
    of 16 + 1 and of 2 + 15 bytes move the offset by 17, members of 17, 31 and 33 bytes by an odd step, so 16
    rounds of each pass every residue; then the ISIZEs at which the CRC32's slice size steps."""
    sizes = [16, 1] * 16 + [2, 15] * 16 + [17] * 16 + [31] * 16 + [33] * 16 + list(ALIGN_STEPS)
    r = random.Random(23)
    pairs = []
    for k, n in enumerate(sizes):
        data = r.randbytes(n) if k % 2 else bytes(r.choices(b"AC", k=n))
        pairs.append((deflate(data, level=(6, 0, 9, 1)[k % 4], strategy=zlib.Z_FIXED if k % 3 == 0 else zlib.Z_DEFAULT_STRATEGY),
                      data))
    return file_of(pairs)


@functools.lru_cache(maxsize=None)
def _three_good():
    text = _texty(7, 90000)
    return [good_member(text[k:k + 30000]) for k in (0, 30000, 60000)]


def _as_second(m: bytes) -> bytes:
    g = _three_good()
    return g[0] + m + g[2] + EOF_MARKER


@functools.lru_cache(maxsize=None)
def written_malformed_cases():
    """name -> (file, the 0-based member the message names, the BgzfError code): one bad member between two good
    ones, as in malformed_cases(). zlib refuses the stream of every case but the ERR_COUNT ones, whose streams
    are well formed and whose ISIZE is wrong."""
    import deflate_writer as W
    out = {}

    def add(name, stream, code, isize=100, crc=0):
        stream = stream.bytes() if isinstance(stream, Bits) else stream
        out[name] = (_as_second(member(stream, crc, isize)), 1, code)

    def pad(bits):
        return bits.put(0, 32)
    lit8 = {s: 3 for s in (97, 98, 99, 100, 256, 257, 258, 259)}
    dist8 = {d: 3 for d in range(8)}
    fl, fd = W.canonical(W.FIXED_LIT), W.canonical(W.FIXED_DIST)
    some = list(b"abcdabcd")

    # ERR_STREAM
    add("fixed_symbol_286", pad(W.body(Bits().put(1, 1).put(1, 2), some, fl, fd, end=False).code(*fl[286])), ERR_STREAM)
    b = W.body(Bits().put(1, 1).put(1, 2), some, fl, fd, end=False).code(*fl[257]).code(*fd[30])
    add("fixed_distance_30", pad(b), ERR_STREAM)
    add("btype_3", pad(W.fixed(Bits(), some, False).put(1, 1).put(3, 2)), ERR_STREAM)
    add("stored_nlen_wrong", W.stored(Bits(), b"stored bytes", True, nlen_xor=0xFFFE), ERR_STREAM)
    cl = {3: 1, 16: 2, 18: 2}
    b = W.header(Bits(), True, 3, 7, cl, [(16, 3)] + [(3, 0)] * 262)
    add("run_16_first", pad(b), ERR_STREAM)
    tokens = W.run_lengths([lit8.get(s, 0) for s in range(260)] + [3] * 8)
    assert tokens[-1] == (16, 2)                 # the last run, made one longer than the array has room for
    b = W.header(Bits(), True, 3, 7, W.code_length_code(tokens), tokens[:-1] + [(16, 3)])
    add("run_past_the_end", pad(W.body(b, some, W.canonical(lit8), W.canonical(dist8))), ERR_STREAM)
    add("hlit_30", pad(W.dynamic(Bits(), some, lit8, dist8, True, nlen=287)), ERR_STREAM)
    add("hdist_30", pad(W.dynamic(Bits(), some, lit8, dist8, True, ndist=31)), ERR_STREAM)
    no_end = {s: 3 for s in (97, 98, 99, 100, 101, 257, 258, 259)}
    b = W.body(W.dynamic_header(Bits(), no_end, dist8, True), some, W.canonical(no_end), W.canonical(dist8), end=False)
    add("no_end_of_block", pad(b), ERR_STREAM)
    three = {97: 2, 98: 2, 256: 2}
    b = W.body(W.dynamic_header(Bits(), three, dist8, True), list(b"abab"), W.canonical(three), W.canonical(dist8))
    add("incomplete_literal_set", pad(b), ERR_STREAM)
    b = W.body(W.dynamic_header(Bits(), lit8, {}, True, ndist=1), some, W.canonical(lit8), {}, end=False)
    add("match_without_distance_code", pad(b.code(*W.canonical(lit8)[257])), ERR_STREAM)
    b = W.body(W.dynamic_header(Bits(), lit8, {2: 1}, True), some, W.canonical(lit8), {}, end=False)
    add("absent_code_of_one_code_set", pad(b.code(*W.canonical(lit8)[257]).put(1, 1)), ERR_STREAM)

    # ERR_EARLY
    add("stored_len_past_input", W.stored(Bits(), b"0123456789", True).bytes()[:-3], ERR_EARLY)
    add("last_block_never_marked", W.fixed(W.fixed(Bits(), some, False), some, False), ERR_EARLY)
    lit15, dist15 = _deep15_lens()
    head = W.dynamic_header(Bits(), lit15, dist15, True)
    whole = W.body(W.dynamic_header(Bits(), lit15, dist15, True), list(b"ACGT"), W.canonical(lit15), W.canonical(dist15))
    assert head.n > 8 * 12
    for cut in (1, 2, 3, 5, 8, (head.n + 7) // 8 - 1):
        add(f"header_cut_at_{cut}" if cut <= 8 else "header_cut_a_byte_before_its_end", whole.bytes()[:cut], ERR_EARLY)

    # ERR_DISTANCE
    raw = _rng_bytes(22, 20000)
    add("distance_one_past_the_start", W.fixed(W.stored(Bits(), raw, False), [(258, 20001), 120], True), ERR_DISTANCE,
        isize=20259)

    # ERR_COUNT: zlib accepts the stream
    def count(name, stream, data, isize):
        assert zlib_verdict(stream.bytes()) == data and isize < len(data)
        add(name, stream, ERR_COUNT, isize=isize, crc=zlib.crc32(data[:isize]))
    count("stored_larger_than_isize", W.stored(Bits(), raw[:500], True), raw[:500], 499)
    toks = list(raw[:40])
    count("literal_at_isize", W.fixed(Bits(), toks, True), W.expand(toks), 39)
    toks = list(raw[:300]) + [(258, 300)]
    count("match_across_isize", W.fixed(Bits(), toks, True), W.expand(toks), 400)
    stream, data = written_cases()["one_distance_code"]
    out["one_distance_code_isize_one_short"] = (_as_second(member(stream, zlib.crc32(data[:-1]), len(data) - 1)), 1, ERR_COUNT)
    return out


GOLDEN_LIBDEFLATE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libdeflate_members.npz")


@functools.lru_cache(maxsize=None)
def libdeflate_members():
    """[(name, raw DEFLATE stream, its bytes)] of tests/golden/libdeflate_members.npz, which
    tests/golden/make_libdeflate_golden.py wrote with libdeflate; the library is not needed to read it."""
    import numpy as np
    g = np.load(GOLDEN_LIBDEFLATE, allow_pickle=False)
    names, of = [n.decode() for n in g["names"]], g["stream_off"]
    plain = {n.decode(): g["plain"][g["plain_off"][k]:g["plain_off"][k + 1]].tobytes() for k, n in enumerate(g["inputs"])}
    return [(n, g["streams"][of[k]:of[k + 1]].tobytes(), plain[n.rsplit("_level_", 1)[0]]) for k, n in enumerate(names)]


def libdeflate_inputs():
    """name -> bytes: what make_libdeflate_golden.py compresses."""
    import genome_cases as GC
    whole = inflate(to_bam(GC.genome()["sam"]))
    text = _texty(31, 70300)
    return dict(texty_65000=text[:65000], texty_5000=text[65000:70000], texty_300=text[70000:], acgt=_rng_bytes(32, 40000, b"ACGT"),
                run=b"z" * 65536, ab=b"ab" * 30000, all_bytes=bytes(range(256)), bam=whole[:60000])


@functools.lru_cache(maxsize=None)
def mutant_seeds():
    """Small well-formed streams of 40 to 3 000 bytes: zlib at levels 1, 6 and 9 and with Z_FIXED, the writer's, the
    fixture's."""
    out = []
    for k, n in enumerate((150, 400, 900, 2000, 4000, 7000)):
        data = _texty(40 + k, n)
        out += [deflate(data, level=1), deflate(data, level=6), deflate(data, level=9), deflate(data, strategy=zlib.Z_FIXED)]
    out += [s for s, _ in written_cases().values()]
    out += [s for _, s, _ in libdeflate_members()]
    out = [s for s in out if 40 <= len(s) <= 3000]
    assert len(out) >= 30
    return out


@functools.lru_cache(maxsize=None)
def mutants(n: int, seed: int):
    """n streams [(stream, zlib's bytes or None)]: a seed with 1 to 3 edits, each a bit flip (half of them in the
    first 60 bytes), a truncation or a byte replaced. The verdict is zlib_verdict()'s."""
    r = random.Random(seed)
    seeds, out = mutant_seeds(), []
    for _ in range(n):
        s = bytearray(r.choice(seeds))
        for _ in range(r.randint(1, 3)):
            kind = r.random()
            if kind < 0.6:
                at = r.randrange(min(60, len(s))) if r.random() < 0.5 else r.randrange(len(s))
                s[at] ^= 1 << r.randrange(8)
            elif kind < 0.75:
                del s[r.randrange(max(1, len(s) - 40), len(s)):]
            else:
                s[r.randrange(len(s))] = r.randrange(256)
            if not s:
                s = bytearray(b"\0")
        out.append((bytes(s), zlib_verdict(bytes(s))))
    return out


# what hc_bgzf_inflate's message says behind "member K at offset N: " for a stream's error
ERR_TEXT = {ERR_STREAM: "a malformed DEFLATE stream", ERR_EARLY: "the DEFLATE stream ends early",
            ERR_COUNT: "the DEFLATE stream does not produce ISIZE bytes",
            ERR_DISTANCE: "a back-reference before the member's first byte"}


@functools.lru_cache(maxsize=None)
def device_refusals(kind: str):
    """The malformed inputs of the device tests, in groups that one child process takes in turn:
    [[(name, file, the texts the message may end with)]]. "written": written_malformed_cases() in 4 groups;
    "mutants": the first 64 mutants of mutants(2000, 1) that zlib refuses, each between two good members, in 4
    groups of 16 (ERR_COUNT only where zlib_overflows() says so)."""
    if kind == "written":
        rows = [(name, file, (ERR_TEXT[code],)) for name, (file, _, code) in sorted(written_malformed_cases().items())]
        size = 7
    else:
        refused = [(k, s) for k, (s, d) in enumerate(mutants(2000, 1)) if d is None][:64]
        rows = [(f"mutant {k}", _as_second(mutant_member(s, None)),
                 tuple(ERR_TEXT[c] for c in (ERR_STREAM, ERR_EARLY, ERR_DISTANCE) + ((ERR_COUNT,) if zlib_overflows(s) else ())))
                for k, s in refused]
        size = 16
        assert len(rows) == 64
    return [rows[k:k + size] for k in range(0, len(rows), size)]


def mutant_member(stream: bytes, data) -> bytes:
    """A mutant as a member: zlib's CRC32 and ISIZE where zlib accepts it; ISIZE 65 536 where it does not, so
    that the inflater walks the stream as far as it goes."""
    return member(stream, 0, 65536) if data is None else member(stream, zlib.crc32(data), len(data))


# ---- BAM -------------------------------------------------------------------------------

def record(ref_id=0, pos=99, mapq=60, flag=0, cigar=(), next_ref_id=-1, next_pos=-1, tlen=0, name=b"q", seq="", qual=None,
           bin_=4680, block_size=None, l_read_name=None, n_cigar=None, l_seq=None, tail=b""):
    """One alignment record. cigar: BAM words; seq: letters of SEQ_CODES; qual: the qualities as they are stored
    (no 33 added), None for 0xFF bytes. The keyword overrides write a field that disagrees with the body."""
    name = bytes(name) + b"\0"
    nib = [SEQ_CODES.index(c) for c in seq] + [0]
    packed = bytes(nib[k] << 4 | nib[k + 1] for k in range(0, len(seq), 2))
    q = b"\xff" * len(seq) if qual is None else bytes(qual)
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) if l_read_name is None else l_read_name, mapq, bin_,
                       len(cigar) if n_cigar is None else n_cigar, flag, len(seq) if l_seq is None else l_seq, next_ref_id,
                       next_pos, tlen)
    body += name + b"".join(struct.pack("<I", w) for w in cigar) + packed + q + tail
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def bam_stream(header_text: bytes, refs, records, magic=b"BAM\x01") -> bytes:
    out = magic + struct.pack("<i", len(header_text)) + header_text + struct.pack("<i", len(refs))
    for name, length in refs:
        n = (name.encode("latin-1") if isinstance(name, str) else bytes(name)) + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", length)
    return out + b"".join(records)


def _fields(line: str):
    f = line
    for c in SPACE:
        f = f.replace(c, " ")
    return f.split()


def split_sam(text: bytes):
    """(header text, [the eleven fields of every alignment line]) as the SAM parser splits a text."""
    lines = text.decode("latin-1").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    k = 0
    while k < len(lines) and lines[k].startswith("@"):
        k += 1
    header = "".join(ln + "\n" for ln in lines[:k])
    return header.encode("latin-1"), [f[:11] for f in map(_fields, lines[k:]) if f]


def representable(f) -> bool:
    """Whether BAM can hold the line's eleven fields as they are."""
    if len(f) < 11 or not all(x.isdigit() for x in (f[1], f[3], f[4], f[7])):
        return False
    if int(f[1]) > 65535 or int(f[4]) > 255 or not 0 <= int(f[3]) <= 2 ** 31 or not 0 <= int(f[7]) <= 2 ** 31:
        return False
    if f[9] == "*" or any(c not in SEQ_CODES for c in f[9]):
        return False
    return f[10] == "*" or (len(f[10]) == len(f[9]) and all(33 <= ord(c) <= 126 for c in f[10]))


def cigar_words(token: str):
    if token == "*":
        return []
    out, n = [], ""
    for c in token:
        if c.isdigit():
            n += c
        else:
            out.append(int(n) << 4 | CIGAR_OPS.index(c))
            n = ""
    return out


def refs_of(fields):
    """The names of RNAME and RNEXT in order of first appearance, each with length 0."""
    seen = []
    for f in fields:
        for name in (f[2], f[6]):
            if name not in ("*", "=") and name not in seen:
                seen.append(name)
    return [(n, 0) for n in seen]


def to_bam(sam_text: bytes, ref_names_and_lengths=None, member_size=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY,
           mem_level=8, compress=None) -> bytes:
    header, fields = split_sam(sam_text)
    refs = refs_of(fields) if ref_names_and_lengths is None else list(ref_names_and_lengths)
    where = {(n if isinstance(n, str) else n.decode("latin-1")): k for k, (n, _) in enumerate(refs)}
    recs = []
    for f in fields:
        assert representable(f), f[:9]
        rid = where.get(f[2], -1) if f[2] != "*" else -1
        nid = rid if f[6] == "=" else -1 if f[6] == "*" else where[f[6]]
        recs.append(record(ref_id=rid, pos=int(f[3]) - 1, mapq=int(f[4]), flag=int(f[1]), cigar=cigar_words(f[5]),
                           next_ref_id=nid, next_pos=int(f[7]) - 1, tlen=int(f[8]), name=f[0].encode("latin-1"), seq=f[9],
                           qual=None if f[10] == "*" else bytes(ord(c) - 33 for c in f[10])))
    return bgzf(bam_stream(header, refs, recs), member_size, level, strategy, mem_level, compress=compress)


def parse_bam(stream: bytes):
    """(header text, refs, [record dict]) of an inflated BAM stream."""
    assert stream[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", stream, 4)
    text = stream[8:8 + l_text]
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, at)
        refs.append((stream[at + 4:at + 4 + l_name - 1].decode("latin-1"), struct.unpack_from("<i", stream, at + 4 + l_name)[0]))
        at += 8 + l_name
    recs = []
    while at < len(stream):
        size, rid, pos, l_name, mapq, _, n_cigar, flag, l_seq, nid, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", stream, at)
        p = at + 36
        name = stream[p:p + l_name - 1]
        p += l_name
        cigar = struct.unpack_from(f"<{n_cigar}I", stream, p)
        p += 4 * n_cigar
        packed = stream[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(SEQ_CODES[packed[k >> 1] >> 4 if k % 2 == 0 else packed[k >> 1] & 15] for k in range(l_seq))
        qual = stream[p:p + l_seq]
        recs.append(dict(ref_id=rid, pos=pos, mapq=mapq, flag=flag, cigar=cigar, next_ref_id=nid, next_pos=npos, tlen=tlen,
                         name=name, seq=seq, qual=qual))
        at += 4 + size
    return text, refs, recs


def sam_of(bam: bytes) -> bytes:
    text, refs, recs = parse_bam(inflate(bam))
    out = [text.decode("latin-1")]
    if out[0] and not out[0].endswith("\n"):
        out[0] += "\n"

    def name_of(k):
        return refs[k][0] if k >= 0 else "*"
    for r in recs:
        cigar = "".join(f"{w >> 4}{CIGAR_OPS[w & 15]}" for w in r["cigar"]) or "*"
        rnext = "=" if r["next_ref_id"] == r["ref_id"] and r["ref_id"] >= 0 else name_of(r["next_ref_id"])
        qual = "*" if not r["qual"] or r["qual"][0] == 0xFF else "".join(chr(q + 33) for q in r["qual"])
        out.append("\t".join(str(x) for x in (r["name"].decode("latin-1"), r["flag"], name_of(r["ref_id"]), r["pos"] + 1,
                                              r["mapq"], cigar, rnext, r["next_pos"] + 1, r["tlen"], r["seq"] or "*", qual))
                   + "\n")
    return "".join(out).encode("latin-1")
