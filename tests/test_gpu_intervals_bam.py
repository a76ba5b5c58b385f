"""GPU: hc_bam_genome_call_intervals (include/hc_intervals.h) without an index on
the shuffled twelve-contig BAM of test_gpu_bam_genome.py, whose header lists the
references in the reverse of the table's order: the call equals the SAM interval
call on sam_of(bam) in every window field, site field and likelihood bit, the
VCF bytes and the records (but line, seq_off, qual_off and line_no), and it
equals the plain BAM call filtered in Python by the stand-in rule. Dense and
sorted buckets, small members and the bases buffer. Then with an index
(bai_writer.py) on the same reads sorted by position, in members of 4 096 and
1 024 bytes, and on the designed big contig of intervals_cases.py: the indexed
call equals the unindexed one by the rule of the header, reads no more members
than the restated query of intervals_restate.py plus the header's, fewer than
half of the big contig's, and uploads fewer bytes than the file has; error
messages carry the virtual offset; BAI errors; a foreign index."""
import numpy as np
import pytest

import bam_cases as BC
import genome_cases as GC
import hcbam
import hcintervals
import hcphmm
import intervals_cases as IC

pytestmark = pytest.mark.gpu

RECORD_FIELDS = ("seq_len", "qual_len", "pos", "cigar", "n_cigar", "flag", "mapq", "mate_same_contig", "defect")


@pytest.fixture(scope="module")
def g():
    return GC.genome()


@pytest.fixture(scope="module")
def refs(g):
    return [(n, len(r)) for n, r in reversed(g["contigs"])]


@pytest.fixture(scope="module")
def bam(g, refs):
    return BC.to_bam(g["sam"], refs, member_size=65280)


@pytest.fixture(scope="module")
def text(bam):
    return BC.sam_of(bam)


@pytest.fixture(scope="module")
def intervals(g):
    names = [n for n, _ in g["contigs"]]
    return IC.by_name(names, ("chrU", GC.VARIANT_AT + 1, GC.VARIANT_AT + 2), ("chrT", 300, 800), ("chrT", 700, 1000),
                      ("chrS246", 245, 246), ("chrF", 8990, 9000))


@pytest.fixture(scope="module")
def plain(engine, g, bam):
    return hcbam.call_genome_bam(bam, g["contigs"], seed=20261020, skip_unplaced=True, want_site_reads=True)


def _same_records(a, e, t):
    ra, re_ = a["sam"]["records"], e["sam"]["records"]
    assert len(ra) == len(re_)
    for f in RECORD_FIELDS:
        assert ra[f].tolist() == re_[f].tolist(), f
    assert a["sam"]["pool"].tolist() == e["sam"]["pool"].tolist()
    assert a["sam"]["contig_of"].tolist() == e["sam"]["contig_of"].tolist()
    assert a["sam"]["line_no"].tolist() == list(range(1, len(ra) + 1))
    for k in (0, len(ra) // 2, len(ra) - 1):
        assert hcbam.hccontig.seq(a["bases"], ra[k]) == hcbam.hccontig.seq(t, re_[k])
        assert hcbam.hccontig.qual(a["bases"], ra[k]) == hcbam.hccontig.qual(t, re_[k])


def test_the_expected_side_keeps_and_drops_lines(plain, g, intervals):
    e = IC.expected(plain, g["contigs"], intervals)
    kept = e["vcf"].split(b"\n")[IC.HEADER_LINES:-1]
    assert 1 <= len(kept) < plain["vcf"].count(b"\n") - IC.HEADER_LINES
    assert len([s for s in e["sites"] if s["status"] == IC.EMITTED]) > len(kept)        # chrU's site: asked, beside the interval
    assert 0 < len(e["asked"]) < len(plain["windows"])


@pytest.mark.parametrize("srt", [False, True])
def test_the_bam_interval_call_equals_the_sam_interval_call(plain, g, bam, text, intervals, srt):
    a = hcintervals.call_genome_bam(bam, g["contigs"], intervals, seed=20261020, want_site_reads=True, sorted_buckets=srt)
    e = hcintervals.call_genome(text, g["contigs"], intervals, seed=20261020, want_site_reads=True, sorted_buckets=srt)
    IC.assert_call(a, e, srt)
    _same_records(a, e, text)
    IC.assert_call(a, IC.expected(plain, g["contigs"], intervals), srt)
    assert a["bases"] == plain["bases"]


def test_small_members_and_whole_contigs(plain, g, refs, text):
    small = BC.to_bam(g["sam"], refs, member_size=4096, level=1)
    assert BC.sam_of(small) == text
    a = hcintervals.call_genome_bam(small, g["contigs"], IC.whole(g["contigs"]), seed=20261020, want_site_reads=True)
    assert a["vcf"] == plain["vcf"] and a["windows"] == plain["windows"] and a["contigs"] == plain["contigs"]
    IC.assert_sites(a["sites"], plain["sites"])
    for k in ("records", "line_no", "pool", "contig_of"):
        assert a["sam"][k].tobytes() == plain["sam"][k].tobytes(), k
    assert a["bases"] == plain["bases"]


def test_a_truncated_file_is_named_and_the_engine_stays_usable(plain, g, bam, intervals):
    with pytest.raises(hcintervals.IntervalError) as e:
        hcintervals.call_genome_bam(bam[:-40], g["contigs"], intervals)
    assert e.value.code == hcphmm.EINVAL and "member" in e.value.msg, e.value.msg
    a = hcintervals.call_genome_bam(bam, g["contigs"], intervals, seed=20261020, want_site_reads=True)
    IC.assert_call(a, IC.expected(plain, g["contigs"], intervals))
    assert a["index_stats"] == dict(chunks=0, members=0, bytes_up=0, records=0)


# ---- with an index ---------------------------------------------------------------------------------

def _identity(r, k):
    """What names record k of result r whatever its index: the fields of the rule in hc_intervals.h."""
    rec = r["sam"]["records"][k]
    words = tuple(r["sam"]["pool"][int(rec["cigar"]):int(rec["cigar"]) + int(rec["n_cigar"])].tolist())
    return (int(rec["pos"]), int(rec["flag"]), int(rec["mapq"]), int(rec["mate_same_contig"]), words,
            hcbam.hccontig.seq(r["bases"], rec), hcbam.hccontig.qual(r["bases"], rec))


def _assert_indexed_equals_unindexed(a, e, what=None):
    """Every window field, site field and bit and the VCF bytes; picked and reads name equal records of their own lists."""
    assert a["merged"] == e["merged"] and a["asked"] == e["asked"], what
    assert len(a["windows"]) == len(e["windows"]), what
    for k, (x, y) in enumerate(zip(a["windows"], e["windows"])):
        for f in IC.WINDOW_FIELDS:
            if f in ("picked", "reads"):
                assert [_identity(a, i) for i in x[f]] == [_identity(e, i) for i in y[f]], (what, k, f)
            else:
                assert x[f] == y[f], (what, k, f, x[f], y[f])
    IC.assert_sites(a["sites"], e["sites"])
    assert a["vcf"] == e["vcf"], what
    n = len(a["sam"]["records"])
    assert a["sam"]["line_no"].tolist() == list(range(1, n + 1)) and a["index_stats"]["records"] == n


def _both(f, intervals, **kw):
    a = hcintervals.call_genome_bam(f["bam"], f["contigs"], intervals, index=f["bai"], seed=20261020, want_site_reads=True, **kw)
    e = hcintervals.call_genome_bam(f["bam"], f["contigs"], intervals, seed=20261020, want_site_reads=True, **kw)
    return a, e


def _assert_stats(f, intervals, a):
    chosen, header, every = IC.restated_members(f, intervals)
    st = a["index_stats"]
    assert 0 < st["members"] <= len(chosen) + len(header), (st, len(chosen), len(header))
    assert st["bytes_up"] < len(f["bam"]) and st["chunks"] >= 1 and st["records"] <= len(BC.split_sam(f["sam"])[1])
    return st, len(every)


@pytest.mark.parametrize("member_size,srt", [(4096, False), (4096, True), (1024, False)])
def test_the_indexed_call_equals_the_unindexed_call_on_the_sorted_genome(engine, intervals, member_size, srt):
    f = IC.sorted_genome(member_size)
    intervals = intervals + IC.by_name([n for n, _ in f["contigs"]], ("chrU", GC.VARIANT_AT, GC.VARIANT_AT + 1))
    a, e = _both(f, intervals, sorted_buckets=srt)
    assert e["vcf"].count(b"\n") > IC.HEADER_LINES + 1 and len({ln.split(b"\t")[0] for ln in e["vcf"].split(b"\n")[4:-1]}) >= 2
    _assert_indexed_equals_unindexed(a, e, (member_size, srt))
    st, every = _assert_stats(f, intervals, a)
    assert st["members"] < every and st["records"] < len(e["sam"]["records"])
    # the whole table asked: every placed record is framed
    w, we = _both(f, IC.whole(f["contigs"]))
    _assert_indexed_equals_unindexed(w, we)
    assert w["index_stats"]["records"] == len(we["sam"]["records"])


@pytest.mark.parametrize("name", sorted(IC.BIG_SETS))
def test_the_big_contig_reads_fewer_than_half_of_the_members(engine, name):
    f = IC.big_contig()
    intervals = IC.BIG_SETS[name]
    a, e = _both(f, intervals)
    assert any(w["picked"] for w in e["windows"]) and e["vcf"].count(b"\n") >= IC.HEADER_LINES + (name != "straddlers")
    _assert_indexed_equals_unindexed(a, e, name)
    st, every = _assert_stats(f, intervals, a)
    assert st["members"] < every / 2, (st, every)
    assert all(e["windows"][w]["picked"] for w in e["asked"])
    if name == "straddlers":
        picked = {int(e["sam"]["records"][k]["pos"]) - 1 for w in e["asked"] for k in e["windows"][w]["picked"]}
        assert picked == {s - 30 for s in IC.STRADDLERS}


def test_a_defective_read_is_named_with_its_virtual_offset(engine):
    f = IC.big_contig()
    at = IC.CLUSTERS[3] + 61
    lines = f["sam"].decode().split("\n")
    k = next(i for i, ln in enumerate(lines) if not ln.startswith("@") and int(ln.split("\t")[3]) > at)
    bad = IC.SC.line(qname="bad", rname="chrBig", pos=at, cigar="59M", seq="A" * 60, flag=99)
    bam = BC.to_bam("\n".join(lines[:k] + [bad] + lines[k:]).encode(), f["refs"], member_size=1024)
    bai = IC.BW.build(bam)
    mem, _, _, recs = IC.BW.layout(bam)
    n = k - 2                                                             # two header lines: the ordinal in the whole file, 0-based
    v = IC.BW.voffset(mem, recs[n][0])
    msgs = []
    for index in (bai, None):
        with pytest.raises(hcintervals.IntervalError) as e:
            hcintervals.call_genome_bam(bam, f["contigs"], IC.BIG_SETS["one_cluster"], index=index)
        assert e.value.code == hcphmm.EINVAL
        msgs.append(e.value.msg)
    assert msgs[1] == f"record {n + 1}: a read that passes the flag filters has the CIGAR's read length differs from seq_len"
    assert msgs[0].endswith(msgs[1].split(": ", 1)[1]) and f"(virtual offset {v}): " in msgs[0] and msgs[0].startswith("record ")
    # out of the intervals it raises nothing, with and without the index
    a, e = (hcintervals.call_genome_bam(bam, f["contigs"], IC.BIG_SETS["straddlers"], index=i, seed=20261020, want_site_reads=True)
            for i in (bai, None))
    _assert_indexed_equals_unindexed(a, e)


def test_bai_errors_come_before_any_record(engine, intervals):
    f = IC.sorted_genome(4096)
    for bad, text in ((b"BAM\x01" + f["bai"][4:], "BAI: missing"), (f["bai"][:100], "BAI: cut short"), (b"", "BAI: cut short"),
                      (IC.BW.pack(IR_refs(f)[:-1]), "BAI: n_ref is 11, the BAM header has 12")):
        with pytest.raises(hcintervals.IntervalError) as e:
            hcintervals.call_genome_bam(f["bam"], f["contigs"], intervals, index=bad)
        assert e.value.code == hcphmm.EINVAL and e.value.msg.startswith(text), e.value.msg
    a, e = _both(f, intervals)
    _assert_indexed_equals_unindexed(a, e)


def IR_refs(f):
    return IC.IR.parse_bai(f["bai"])


def test_a_foreign_index_gives_an_error_or_a_result_and_the_engine_lives(engine, intervals):
    """The .bai of the same reads in members of another size: its offsets lie inside this file, its chunks begin
    where this file has no record. Whatever comes back, nothing is read out of bounds and the next call is right."""
    f, other = IC.sorted_genome(4096), IC.sorted_genome(1024)
    foreign = [(bins, linear) for bins, linear in IC.IR.parse_bai(other["bai"])]
    top = max((c[1] >> 16 for bins, _ in foreign for cs in bins.values() for c in cs), default=0)
    for bai, bam in ((IC.BW.pack(foreign), f["bam"] + bytes(max(0, top + 1 - len(f["bam"])))), (f["bai"], other["bam"])):
        try:
            r = hcintervals.call_genome_bam(bam, f["contigs"], intervals, index=bai)
            assert len(r["windows"]) == 76
        except hcintervals.IntervalError as e:
            assert e.code == hcphmm.EINVAL, e.msg
    a, e = _both(f, intervals)
    _assert_indexed_equals_unindexed(a, e)


def test_chunks_packed_across_the_staging_blocks_border(engine, monkeypatch, intervals):
    """A staging block of 4 096 bytes: the chunks' stretches of members are cut where the block is full, and a stretch
    begins in the middle of a block."""
    f = IC.sorted_genome(1024)
    a, e = _both(f, intervals)
    assert a["index_stats"]["chunks"] >= 2 and a["index_stats"]["bytes_up"] > 3 * 4096, a["index_stats"]
    monkeypatch.setenv("HC_SAM_STAGE_BYTES", "4096")
    b, _ = _both(f, intervals)
    _assert_indexed_equals_unindexed(b, e)
    assert b["index_stats"] == a["index_stats"] and b["bases"] == a["bases"]
    for k in ("records", "line_no", "pool", "contig_of"):
        assert a["sam"][k].tobytes() == b["sam"][k].tobytes(), k
