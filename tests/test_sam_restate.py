"""CPU: the restatement (sam_restate.py) pinned to cases worked by hand from the
reference's text (sam.hpp:100-114, cigar.hpp:57-68, haplotypecaller.hpp:24-50,
112-154, variant.hpp:31-44), and the shared inputs of sam_cases.py checked for
what they claim to contain."""
import pytest

import sam_cases as SC
import sam_restate as SR

REC = "r1\t99\tchrT\t7\t60\t2S3M1D1M\t=\t150\t-250\tACGTAC\tIIIIII"


def test_extraction_skips_whitespace_and_stops_at_it():
    assert SR.extract("  ab\tcd", 0) == ("ab", 2, 4)
    assert SR.extract("  ab\tcd", 4) == ("cd", 5, 7)
    assert SR.extract("ab \v\f\r", 2) == (None, 6, 6)


def test_one_record_by_hand():
    # offsets: r1=0 99=3 chrT=6 7=11 60=13 CIGAR=16 '='=25 150=27 -250=31 SEQ=36 QUAL=43
    r = SR.parse_record(REC)
    assert (r["flag"], r["pos"], r["mapq"], r["mate_same_contig"]) == (99, 7, 60, 1)
    assert r["elements"] == [(2, "S"), (3, "M"), (1, "D"), (1, "M")] and r["n_cigar"] == 4
    assert (r["seq_off"], r["seq_len"], r["qual_off"], r["qual_len"]) == (36, 6, 43, 6)
    assert r["defect"] == 0          # S + M + M = 6 = len(SEQ)


def test_cigar_words_are_bam_packed():
    # "MIDNSHP=X": S = 4, M = 0, D = 2
    got = SR.load_all_reads(REC)
    assert got["pool"] == [2 << 4 | 4, 3 << 4 | 0, 1 << 4 | 2, 1 << 4 | 0]
    assert SR.to_cigar_elements("*") == [] and SR.to_cigar_elements("10=2X") == [(10, "="), (2, "X")]
    for bad in ("", "M", "3", "3M2", "3Q", "268435456M", "**"):
        assert SR.to_cigar_elements(bad) is None, bad


def test_header_later_at_line_crlf_open_last_line_and_tags():
    rec2 = REC.replace("r1", "@r2").replace("\t7\t", "\t9\t")
    text = "@HD\tVN:1.6\r\n@SQ\tSN:chrT\r\n" + REC + "\tNM:i:1\tXX:Z:a b\r\n" + rec2 + "\r\n\r\n" + REC.replace("\t", " ")
    got = SR.load_all_reads(text.encode())
    assert got["n_header_lines"] == 2
    recs = got["records"]
    assert [r["line_no"] for r in recs] == [3, 4, 6]             # line 5 holds "\r" alone: skipped
    assert [r["pos"] for r in recs] == [7, 9, 7]                 # the later '@' line is a record
    assert recs[0]["line"] == len("@HD\tVN:1.6\r\n@SQ\tSN:chrT\r\n")
    assert recs[0]["qual_len"] == 6                              # neither the tags nor '\r' belong to QUAL
    assert recs[2]["line"] + recs[2]["qual_off"] + recs[2]["qual_len"] == len(text)   # the last line has no newline
    assert [r["cigar"] for r in recs] == [0, 4, 8]
    assert SR.load_all_reads(b"")["records"] == [] and SR.load_all_reads(b"@HD\n@CO\tx")["n_header_lines"] == 2
    assert [x[1] for x in SR.lines_of("a\n\nb\n")] == ["a", "", "b"]


@pytest.mark.parametrize("line,field", [("x", "fields"), (REC.rsplit("\t", 1)[0], "fields"),
                                        (REC.replace("99", "-99"), "FLAG"), (REC.replace("\t7\t", "\t+7\t"), "POS"),
                                        (REC.replace("\t60\t", "\t65536\t"), "MAPQ"), (REC.replace("3M", "3m"), "CIGAR"),
                                        (REC.replace("150", "1e3"), "PNEXT"), (REC.replace("-250", "--250"), "TLEN")])
def test_syntax_errors_name_line_and_field(line, field):
    with pytest.raises(SR.SamSyntax) as e:
        SR.load_all_reads(("@HD\n" + REC + "\n" + line + "\nx\n").encode())
    assert (e.value.line_no, e.value.field) == (3, field)


def test_defects_in_their_order():
    def d(**kw):
        return SR.parse_record(SC.line(**kw))["defect"]
    assert d() == 0 and d(pos=0, cigar="*") == 1 and d(cigar="*", qual="I") == 2 and d(cigar="3M", qual="I") == 3
    assert d(qual="III") == 4 and d(seq="A" * 65537) == 5 and d(seq="A" * 65536) == 0
    assert d(cigar="4M9H9D9N9P") == 0      # H D N P do not count towards the read length


def test_window_bounds_by_hand():
    # 12 x 245 + 47 bases: 13 windows; window 0 has no left padding, the last origin runs past the contig
    b = SR.window_bounds(2987)
    assert len(b) == 13
    assert b[0] == (0, 330, 0, 245) and b[1] == (160, 575, 245, 490) and b[12] == (2855, 3270, 2940, 3185)
    assert SR.window_bounds(245) == [(0, 330, 0, 245)] and len(SR.window_bounds(246)) == 2
    assert SR.window_bounds(30, 10, 3) == [(0, 13, 0, 10), (7, 23, 10, 20), (17, 33, 20, 30)]


def test_picks_by_hand():
    # ref_len 30, region 10, padding 3: position 8 lies in windows 0 and 1, 29 in window 2, 30 holds no reads
    rmap = {8: [4, 1, 7], 12: [2], 29: [0, 9], 30: [5]}
    calls = []

    def last(w, b, c):
        calls.append((w, b, c))
        return c - 1
    assert SR.picks(rmap, 30, 10, 3, last) == [[7, 2], [7, 2], [9]]
    assert calls == [(0, 8, 3), (0, 12, 1), (1, 8, 3), (1, 12, 1), (2, 29, 2)]
    # two windows pick independently in their overlap
    assert SR.picks(rmap, 30, 10, 3, lambda w, b, c: w % c)[:2] == [[4, 2], [1, 2]]
    assert SR.picks(rmap, 30, 10, 3, SR.pick_first) == [[4, 2], [4, 2], [0]]


def test_reads_map_placement():
    recs = SR.load_all_reads("\n".join([SC.line(pos=5), SC.line(pos=3), SC.line(pos=5, mapq=0, cigar="*"), SC.line(pos=0),
                                        SC.line(pos=31)]).encode())["records"]
    with pytest.raises(SR.Unplaced) as e:
        SR.reads_map(recs, 30)
    assert e.value.line_no == 4
    assert SR.reads_map(recs, 30, skip_unplaced=True) == {4: [0, 2], 2: [1]}     # file order; the filtered defect passes
    assert SR.reads_map(recs, 31, skip_unplaced=True) == {4: [0, 2], 2: [1], 30: [4]}
    bad = SR.load_all_reads("\n".join([SC.line(pos=5), SC.line(pos=9, cigar="3M"), SC.line(pos=0)]).encode())["records"]
    with pytest.raises(SR.Defective) as e:
        SR.reads_map(bad, 30)
    assert (e.value.line_no, e.value.defect) == (2, 3)


def test_pick_formula_on_three_hand_computed_cases():
    """Worked with 64-bit integer arithmetic outside the restatement; the first
    is splitmix64's published first output for seed 0, 0xE220A8397B1DCDAF:
    (0xE220A839 * 3) >> 32 = 2."""
    assert SR.pick_seeded(0, 0, 0, 3) == 2
    assert SR.pick_seeded(1, 2, 330, 5) == 3            # z = 0x9FEC741FF92B148F
    assert SR.pick_seeded(2 ** 64 - 1, 12, 2986, 1000) == 549   # z = 0x8CC1E1EAC62CD0E6
    assert all(0 <= SR.pick_seeded(7, w, b, c) < c for w in range(3) for b in range(50) for c in (1, 2, 3, 64))


def test_variant_print_and_header():
    assert SR.VCF_HEADER.splitlines()[3].split("\t") == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO",
                                                         "FORMAT", "NA12878"]
    assert SR.variant_line("chrT", 99, ["A", "C"], (0, 1), 87) == "chrT\t100\t.\tA\tC\t.\t.\t.\tGT:GQ\t0/1:87\n"
    assert SR.variant_line("c", 0, ["AT", "A", "ATT"], (1, 2), 5) == "c\t1\t.\tAT\tA,ATT\t.\t.\t.\tGT:GQ\t1/2:5\n"
    sites = [dict(status=1, begin=3, alleles=[b"A", b"G"], a1=0, a2=0, genotype_quality=9),
             dict(status=0, begin=3, alleles=[b"A", b"G"], a1=1, a2=1, genotype_quality=9)]
    assert SR.vcf("c", sites) == SR.VCF_HEADER + "c\t4\t.\tA\tG\t.\t.\t.\tGT:GQ\t1/1:9\n"


# ---- sam_cases.py holds what it says ------------------------------------------------

def test_grid_covers_every_offset():
    text = SC.texts()["grid"]
    exp = SC.expected("grid")
    starts = [r["line"] for r in exp["records"]]
    assert {s % 64 for s in starts} == set(range(64))
    tokens = {(r["line"] + r[f]) for r in exp["records"] for f in ("seq_off", "qual_off")}
    assert {t % 64 for t in tokens} == set(range(64)) and {t % 16 for t in tokens} == set(range(16))
    newlines = [i for i, c in enumerate(text) if c == 10]
    assert {i % 64 for i in newlines} == set(range(64))
    lengths = {len(x) for x in SC.grid_lines()}
    assert set(range(1, 701)) <= lengths                        # a line of every length from 1 to 700 bytes
    assert all(not x.strip() for x in SC.grid_lines() if 0 < len(x) <= 20)
    assert {len(x) for x in SC.grid_lines() if x.strip()} >= set(range(21, 701))
    assert not text.endswith(b"\n") and len(text) > 3 * 65536


def test_newlines_sit_on_the_chunk_edges():
    """The line scan works on chunks of 1024 bytes and carries "the byte before was
    a newline" from chunk to chunk: newlines on a chunk's last byte and first byte."""
    def at(name):
        return [i for i, c in enumerate(SC.texts()[name]) if c == 10]
    assert at("chunk_edges")[:5] == [1023, 2047, 3072, 4095, 6596]
    assert at("chunk_edges_crlf")[:2] == [1024, 2047] and SC.texts()["chunk_edges_crlf"][1023] == 13
    for name in ("grid", "grid_newline", "grid_crlf", "many_lines"):
        assert any(i % 1024 == 1023 for i in at(name)), name
    many = SC.texts()["many_lines"]
    assert many.count(b"\n") > 2 * 4096 and len(many) > 4096 * 1024      # several scan tiles of lines and of chunks
    assert len(SC.expected("many_lines")["pool"]) > 4096
    assert [r["seq_len"] for r in SC.expected("chunk_edges")["records"]] == [489, 489, 490, 489, 1228, 13]


def test_short_error_lines_of_every_length():
    short = {len(bad): bad for name, bad, _ in SC.error_lines() if name.startswith("short_")}
    assert sorted(short) == list(range(1, 21)) and all(x.strip() and x[0] != " " for x in short.values())


def test_grid_reaches_every_case():
    recs = SC.expected("grid")["records"]
    assert {r["defect"] for r in recs} == {0, 1, 2, 3, 4, 5}
    ops = {w & 15 for w in SC.expected("grid")["pool"]}
    assert ops == set(range(9))
    assert max(r["n_cigar"] for r in recs) == 200 and min(r["n_cigar"] for r in recs) == 0
    assert max(w >> 4 for w in SC.expected("grid")["pool"]) == (1 << 28) - 1
    assert max(r["flag"] for r in recs) == 65535 and max(r["pos"] for r in recs) == 4294967295
    assert {r["mate_same_contig"] for r in recs} == {0, 1}
    assert len(recs) == len([x for x in SC.grid_lines() if x.strip()])
    assert SC.expected("header_only")["records"] == [] and SC.expected("empty")["n_header_lines"] == 0
    assert len(SC.expected("grid_crlf")["records"]) == len(recs)
    assert SC.expected("no_header")["n_header_lines"] == 0


def test_error_texts_fail_in_the_restatement_where_they_say():
    seen = set()
    for name, text, line_no, field in SC.error_texts():
        with pytest.raises(SR.SamSyntax) as e:
            SR.load_all_reads(text)
        assert (e.value.line_no, e.value.field) == (line_no, field), name
        seen.add(field)
    assert seen == set(SC.ERROR_TEXT)


def test_contig_holds_what_the_issue_asks_for():
    c = SC.contig()
    assert len(c["ref"]) == 12 * 245 + 47 and len(SR.window_bounds(len(c["ref"]))) == 13
    parsed = SR.load_all_reads(c["sam"])
    recs = parsed["records"]
    pos = [r["pos"] for r in recs]
    assert pos != sorted(pos)                                           # unsorted in the file
    rmap = SR.reads_map(recs, len(c["ref"]))
    sizes = {len(v) for v in rmap.values()}
    assert {1, 2, 3} <= sizes and len(rmap) < len(c["ref"])             # positions hold 0, 1 or several reads
    assert any(w & 15 == 4 for w in parsed["pool"])                     # soft clips
    bounds = SR.window_bounds(len(c["ref"]))
    per_window = SR.picks(rmap, len(c["ref"]), 245, 85, SR.pick_first)
    assert [bool(p) for p in per_window] == [w != SC.NO_READS_WINDOW for w in range(13)]
    for w, (pb, pe, ob, oe) in enumerate(bounds[:12]):
        if w == SC.NO_READS_WINDOW:
            continue
        mine = [r for r in recs if ob <= r["pos"] - 1 < oe]
        assert any(r["mapq"] < 20 for r in mine) and any(r["flag"] & 0x400 for r in mine), w
        assert any(r["flag"] & 0x100 for r in mine) and any(not r["mate_same_contig"] for r in mine), w
    # two seeds and the first pick give three different selections
    a, b = (SR.picks(rmap, len(c["ref"]), 245, 85, SR.pick_fn("seeded", s)) for s in (0, 1))
    assert a != b and a != per_window
    # overlapping windows pick independently
    assert any(set(a[w]) - set(a[w + 1]) and any(recs[k]["pos"] - 1 >= bounds[w + 1][0] for k in set(a[w]) - set(a[w + 1]))
               for w in range(6))
    # the other order has the same per-position lists
    again = SR.load_all_reads(c["sam_reshuffled"])
    assert c["sam_reshuffled"] != c["sam"]
    names = lambda sam, p: {b: [sam[p["records"][k]["line"]:].split(b"\t", 1)[0] for k in v]
                            for b, v in SR.reads_map(p["records"], len(c["ref"])).items()}
    assert names(c["sam"], parsed) == names(c["sam_reshuffled"], again)
