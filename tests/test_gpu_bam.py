"""GPU: hc_bam_parse (include/hc_bam.h) through hcbam.parse.

The texts of sam_cases.py (the parse grid and the 13-window contig) and of
genome_cases.py, converted with bam_cases.to_bam at member sizes of 64, 4 096
and 65 280 bytes (records, the header and block_size words straddle member
borders): every field of the records equals the SAM parser's parse of
sam_of(bam), the pool word for word, and the bytes the records view in the
bases buffer are the SEQ and QUAL tokens of that text. Lines that BAM cannot
hold (MAPQ above 255, POS above 2^31, SEQ or QUAL "*") are left out of the grid.
The genome text once more in members that zlib did not write (one dynamic block
each from tests/deflate_writer.py, code lengths up to 15). Then what has no SAM twin (l_seq 0, QUAL 0xFF, a quality of 94, all 16 nibble
codes, refID -1, pos -1, an empty BAM) and every BAM error of the header."""
import struct
import zlib

import numpy as np
import pytest

import bam_cases as BC
import genome_cases as GC
import hcbam
import hccontig
import hcphmm
import sam_cases as SC

pytestmark = pytest.mark.gpu

SAME = ("pos", "flag", "mapq", "cigar", "n_cigar", "seq_len", "qual_len", "mate_same_contig", "defect")


def _representable(text: bytes) -> bytes:
    header, fields = BC.split_sam(text)
    keep = [f for f in fields if BC.representable(f) and f[10] != "*"]
    assert len(keep) > 0.9 * len(fields)
    return header + "".join("\t".join(f) + "\n" for f in keep).encode("latin-1")


def _texts():
    return dict(grid=_representable(SC.texts()["grid"]), contig=SC.contig()["sam"], genome=GC.genome()["sam"])


@pytest.fixture(scope="module")
def expected(engine):
    """Per text: (T, the SAM parser's parse of T); T does not depend on the member size."""
    out = {}
    for name, text in _texts().items():
        t = BC.sam_of(BC.to_bam(text))
        out[name] = (t, hccontig.parse_sam(t))
    return out


def test_the_grid_keeps_its_edge_lines():
    """On the expected side."""
    _, fields = BC.split_sam(_texts()["grid"])
    names = {f[0] for f in fields}
    assert {"ops", "long_cigar", "max_len_d", "defect_pos", "defect_no_cigar", "defect_cigar_length", "defect_too_long",
            "just_fits", "other_contig", "last_line_without_newline"} <= names
    assert {len(f[9]) % 2 for f in fields} == {0, 1}


@pytest.mark.parametrize("member_size", [64, 4096, 65280])
@pytest.mark.parametrize("name", ["grid", "contig", "genome"])
def test_records_equal_the_sam_parse_of_the_canonical_text(expected, name, member_size):
    text = _texts()[name]
    bam = BC.to_bam(text, member_size=member_size)
    t, e = expected[name]
    assert BC.sam_of(bam) == t
    if member_size == 64:
        assert len(BC.members(bam)) > len(BC.inflate(bam)) // 64
    g = hcbam.parse(bam)
    assert len(g["records"]) == len(e["records"]) > 100
    for f in SAME:
        assert g["records"][f].tolist() == e["records"][f].tolist(), f
    assert g["pool"].tolist() == e["pool"].tolist()
    assert g["line_no"].tolist() == list(range(1, len(g["records"]) + 1))
    assert (g["records"]["seq_off"] == 0).all() and g["records"]["qual_off"].tolist() == g["records"]["seq_len"].tolist()
    at = 0
    for k, (a, b) in enumerate(zip(g["records"], e["records"])):
        assert int(a["line"]) == at
        assert hccontig.seq(g["bases"], a) == hccontig.seq(t, b), k
        assert hccontig.qual(g["bases"], a) == hccontig.qual(t, b), k
        at += 2 * int(a["seq_len"])
    assert at == len(g["bases"])
    header, fields = BC.split_sam(text)
    assert g["header"] == header and g["refs"] == BC.refs_of(fields)
    where = {n: k for k, (n, _) in enumerate(g["refs"])}
    assert g["ref_id"].tolist() == [where.get(f[2], -1) for f in fields]


def test_members_from_another_writer(expected):
    """The genome text in members that zlib did not write: each one dynamic block from deflate_writer with
    complete(., 15) code lengths over the symbols it uses (bam_cases.written_compress)."""
    import deflate_census as DC
    text = _texts()["genome"]
    bam = BC.to_bam(text, member_size=20000, compress=BC.written_compress)
    t, e = expected["genome"]
    assert BC.sam_of(bam) == t
    ms = BC.members(bam)
    assert 50 < len(ms) < 400
    c = DC.merge(DC.walk(s)[1] for _, s, _, n in ms[:3])
    assert c["block_types"] == {2} and max(c["lit_declared"]) == 15 and max(c["dist_declared"]) == 15 and c["max_distance"] > 10000
    g = hcbam.parse(bam)
    assert len(g["records"]) == len(e["records"]) > 100
    for f in SAME:
        assert g["records"][f].tolist() == e["records"][f].tolist(), f
    assert g["pool"].tolist() == e["pool"].tolist()
    for k, (a, b) in enumerate(zip(g["records"], e["records"])):
        assert hccontig.seq(g["bases"], a) == hccontig.seq(t, b), k
        assert hccontig.qual(g["bases"], a) == hccontig.qual(t, b), k
    header, fields = BC.split_sam(text)
    assert g["header"] == header and g["refs"] == BC.refs_of(fields)
    inflated = hcbam.inflate(bam)
    off = 0
    for k, (_, s, _, n) in enumerate(ms):
        assert inflated["bytes"][off:off + n] == zlib.decompress(s, -15), f"member {k}"
        off += n


def _bam(records, refs=(("chrA", 1000), ("chrB", 50)), header=b"@HD\tVN:1.6\n", member_size=65280):
    return BC.bgzf(BC.bam_stream(header, list(refs), records), member_size=member_size)


def test_what_has_no_sam_twin(engine):
    m = lambda n: [n << 4]                                                  # noqa: E731
    recs = [
        BC.record(seq=BC.SEQ_CODES, cigar=m(16), qual=bytes(range(16))),                  # all 16 codes, even
        BC.record(seq=BC.SEQ_CODES[::-1] + "A", cigar=m(17), qual=bytes([93] * 17)),      # odd, the highest quality text can hold
        BC.record(seq="", cigar=m(5)),                                                    # l_seq 0
        BC.record(seq="ACGT", cigar=m(4), qual=None),                                     # QUAL 0xFF
        BC.record(seq="ACGTA", cigar=m(5), qual=bytes([10, 94, 10, 10, 10])),             # a quality of 94
        BC.record(seq="ACGTA", cigar=m(5), qual=bytes([10, 10, 10, 10, 255])),            # 0xFF not in front: a quality
        BC.record(ref_id=-1, next_ref_id=-1, seq="AC", cigar=m(2), qual=b"\x05\x05"),     # refID -1
        BC.record(pos=-1, seq="AC", cigar=m(2), qual=b"\x05\x05"),                        # pos -1
        BC.record(ref_id=1, next_ref_id=1, seq="AC", cigar=m(2), qual=b"\x05\x05", flag=65535, mapq=255, pos=2 ** 31 - 2),
        BC.record(ref_id=1, next_ref_id=0, seq="A", cigar=[], qual=b"\x05"),
        BC.record(seq="", cigar=[]),
    ]
    g = hcbam.parse(_bam(recs))
    r = g["records"]
    assert r["seq_len"].tolist() == [16, 17, 0, 4, 5, 5, 2, 2, 2, 1, 0]
    assert r["qual_len"].tolist() == [16, 17, 0, 0, 5, 5, 2, 2, 2, 1, 0]
    assert r["defect"].tolist() == [0, 0, hccontig.DEFECT_CIGAR_LENGTH, hccontig.DEFECT_QUAL_LENGTH, hcbam.DEFECT_QUAL_RANGE,
                                    hcbam.DEFECT_QUAL_RANGE, 0, hccontig.DEFECT_POS_ZERO, 0, hccontig.DEFECT_NO_CIGAR,
                                    hccontig.DEFECT_NO_CIGAR]
    assert r["pos"].tolist() == [100] * 7 + [0, 2 ** 31 - 1, 100, 100]
    assert r["mate_same_contig"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert (int(r["flag"][8]), int(r["mapq"][8])) == (65535, 255)
    assert g["ref_id"].tolist() == [0, 0, 0, 0, 0, 0, -1, 0, 1, 1, 0]
    assert hccontig.seq(g["bases"], r[0]) == BC.SEQ_CODES.encode()
    assert hccontig.qual(g["bases"], r[0]) == bytes(range(33, 49))
    assert hccontig.seq(g["bases"], r[1]) == (BC.SEQ_CODES[::-1] + "A").encode()
    assert hccontig.qual(g["bases"], r[1]) == b"~" * 17
    assert g["pool"].tolist() == [16 << 4, 17 << 4, 5 << 4, 4 << 4, 5 << 4, 5 << 4, 2 << 4, 2 << 4, 2 << 4]
    assert r["cigar"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9]
    assert g["refs"] == [("chrA", 1000), ("chrB", 50)] and g["header"] == b"@HD\tVN:1.6\n"


def test_empty_bam(engine):
    g = hcbam.parse(_bam([]))
    assert len(g["records"]) == 0 and len(g["pool"]) == 0 and g["bases"] == b"" and len(g["refs"]) == 2
    g = hcbam.parse(_bam([], refs=(), header=b""))
    assert len(g["records"]) == 0 and g["refs"] == [] and g["header"] == b""


def _fails(bam):
    with pytest.raises(hcbam.BamError) as e:
        hcbam.parse(bam)
    assert e.value.code == hcphmm.EINVAL
    return e.value.msg


def test_bam_errors(engine):
    m = lambda n: [n << 4]                                                  # noqa: E731
    ok = BC.record(seq="ACGT", cigar=m(4), qual=b"\x05" * 4)
    stream = BC.bam_stream(b"@HD\n", [("chrA", 1000), ("chrB", 50)], [ok, ok, ok])

    def with_fourth(rec, member_size=65280):
        return _bam([ok, ok, ok, rec, ok], member_size=member_size)
    assert "BAM header: missing BAM" in _fails(BC.bgzf(BC.bam_stream(b"", [], [], magic=b"BAM\x02")))
    assert "BAM header: missing BAM" in _fails(BC.bgzf(b"BA"))
    assert "BAM header: missing BAM" in _fails(b"")
    for cut in (6, 10, 14, 20, 33):
        assert "BAM header: cut short" in _fails(BC.bgzf(stream[:cut])), cut
    assert _fails(BC.bgzf(stream[:-5])).startswith("record 3: cut short")
    assert _fails(BC.bgzf(stream + b"\x01\x02")).startswith("record 4: cut short")
    assert _fails(with_fourth(BC.record(seq="ACGT", cigar=m(4), block_size=31))).startswith("record 4: block_size smaller")
    small = BC.record(seq="ACGT" * 10, cigar=m(40), block_size=60)
    assert _fails(with_fourth(small)).startswith("record 4: block_size smaller")
    assert _fails(with_fourth(BC.record(seq="AC", cigar=m(2), l_seq=-1))).startswith("record 4: block_size smaller")
    assert _fails(with_fourth(BC.record(seq="ACGT", cigar=[4 << 4 | 9]))).startswith("record 4: a CIGAR op above 8")
    assert _fails(with_fourth(BC.record(seq="ACGT", cigar=[1 << 4, 3 << 4 | 15]), 64)).startswith("record 4: a CIGAR op")
    assert _fails(with_fourth(BC.record(ref_id=2, seq="A", cigar=m(1)))).startswith("record 4: refID outside")
    assert _fails(with_fourth(BC.record(ref_id=-2, seq="A", cigar=m(1)))).startswith("record 4: refID outside")
    assert _fails(with_fourth(BC.record(next_ref_id=2, seq="A", cigar=m(1)))).startswith("record 4: next_refID outside")
    assert _fails(with_fourth(BC.record(seq="A", cigar=m(1), l_read_name=0))).startswith("record 4: l_read_name is 0")
    # the lowest record wins, whichever side finds it
    bad_op, bad_ref = BC.record(seq="ACGT", cigar=[4 << 4 | 9]), BC.record(ref_id=7, seq="A", cigar=m(1))
    assert _fails(_bam([ok, bad_op, ok, bad_ref])).startswith("record 2: a CIGAR op")
    assert _fails(_bam([ok, bad_ref, ok, bad_op])).startswith("record 2: refID")
    # a container error in front of a BAM error
    file = _bam([ok, bad_ref], member_size=40)
    first = BC.members(file)[0]
    broken = file[:len(first[1]) + 18] + struct.pack("<I", first[2] ^ 1) + file[len(first[1]) + 22:]
    assert _fails(broken).startswith("member 0 at offset 0: CRC32 mismatch")
    # raw BAM is not BGZF
    assert _fails(stream).startswith("member 0 at offset 0: not a BGZF member")
    g = hcbam.parse(BC.bgzf(stream, member_size=7))
    assert len(g["records"]) == 3 and np.all(g["records"]["defect"] == 0)
