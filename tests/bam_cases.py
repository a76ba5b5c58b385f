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
"""
from __future__ import annotations

import functools
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


def bgzf(data: bytes, member_size=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, eof=True) -> bytes:
    out = b"".join(good_member(data[k:k + member_size], level=level, strategy=strategy, mem_level=mem_level)
                   for k in range(0, len(data), member_size))
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
    """A DEFLATE bit writer: put() least significant bit first, code() a Huffman code, most significant first."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        self.acc |= value << self.n
        self.n += n
        return self

    def code(self, code, n):
        for k in range(n - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


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
           mem_level=8) -> bytes:
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
    return bgzf(bam_stream(header, refs, recs), member_size, level, strategy, mem_level)


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
