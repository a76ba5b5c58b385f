"""CPU: the restatement of filter_reads / hard_clip_reads (prep_restate.py) pinned
to cases worked by hand from the reference's text (utils/read_clipper.hpp:32-91,
utils/read_filter.hpp, sam/sam.hpp:69-72, sam/cigar.hpp:92-111). They say in
words what the code does at its quirks; what holds the restatement to the
headers themselves is tests/test_ref_pins.py, which compares it with the
reference compiled in place. Coordinates are 0-based begins (POS = begin + 1)."""
import prep_restate as PR

SEQ = PR.make_seq


def _rec(begin, cigar, n, flag=0, mapq=60, rnext="="):
    return PR.SAMRecord(flag, begin + 1, mapq, cigar, rnext, SEQ(n))


def test_1_forward_single_soft_clip_becomes_match():
    r = _rec(100, "50S", 50)
    PR.revert_soft_clipped_bases(r)
    # front: S and 100 >= 50 -> 50M, POS moves left by 50; back() is now 50M, not S: nothing removed
    assert PR.cigar_text(r.CIGAR) == "50M" and r.get_alignment_begin() == 50
    assert r.SEQ == SEQ(50) and r.get_interval() == (50, 100)


def test_2_reverse_single_soft_clip_loses_every_base():
    r = _rec(100, "50S", 50, flag=0x10)
    PR.revert_soft_clipped_bases(r)
    # front: S removes 50 bases, CIGAR alone; back() is the same element, still S -> 50M
    assert r.SEQ == "" and PR.cigar_text(r.CIGAR) == "50M" and r.get_interval() == (100, 150)
    kept, reasons = PR.prepare([_rec(100, "50S", 50, flag=0x10)], 0, 1000)
    assert kept == [] and reasons == [PR.MIN_LENGTH]


def test_3_forward_front_clip_longer_than_begin_is_left_alone():
    r = _rec(10, "20S30M", 50)
    PR.revert_soft_clipped_bases(r)
    assert PR.cigar_text(r.CIGAR) == "20S30M" and r.SEQ == SEQ(50) and r.get_interval() == (10, 40)


def test_4_clip_larger_than_the_read_wraps_and_keeps_it_whole():
    r = _rec(1000, "10M100D10M", 20)
    PR.revert_soft_clipped_bases(r)
    assert r.get_alignment_end() == 1120
    PR.hard_clip_to_interval(r, 900, 1050)
    # clip = 70 > 20: size - clip wraps, substr(0, huge) keeps all 20 bases
    assert r.SEQ == SEQ(20)
    w = dict(begin=900, end=1050, reads=[dict(flag=0, mapq=60, pos=1001, cigar="10M100D10M", mate_same=1, seq_len=20)])
    rec = PR.records(w)["records"][0]
    assert (rec["keep"], rec["offset"], rec["length"]) == (1, 0, 20)


def test_5_front_hard_clip():
    r = _rec(890, "101M", 101)
    PR.hard_clip_to_interval(r, 900, 1300)
    assert r.SEQ == SEQ(101)[10:] and len(r.SEQ) == 91
    assert r.POS == 891 and PR.cigar_text(r.CIGAR) == "101M"   # POS and CIGAR stay


def test_6_read_wholly_before_the_window_is_emptied():
    for before in (101, 102, 500):
        kept, reasons = PR.prepare([_rec(900 - before, "101M", 101)], 900, 1300)
        assert kept == [] and reasons == [PR.MIN_LENGTH]
        r = _rec(900 - before, "101M", 101)
        PR.hard_clip_to_interval(r, 900, 1300)
        assert r.SEQ == ""


def test_7_boundary_pairs():
    # post-clip lengths 9 and 10
    kept, reasons = PR.prepare([_rec(1291, "40M", 40), _rec(1290, "40M", 40)], 900, 1300)
    assert reasons == [PR.MIN_LENGTH, PR.KEPT] and [len(k.SEQ) for k in kept] == [10]
    kept, reasons = PR.prepare([_rec(869, "40M", 40), _rec(870, "40M", 40)], 900, 1300)
    assert reasons == [PR.MIN_LENGTH, PR.KEPT] and kept[0].SEQ == SEQ(40)[30:]
    # MAPQ 19 and 20
    kept, reasons = PR.prepare([_rec(1000, "40M", 40, mapq=19), _rec(1000, "40M", 40, mapq=20)], 900, 1300)
    assert reasons == [PR.MAPQ, PR.KEPT] and len(kept) == 1


def test_filter_order_and_survivor_order():
    reads = [_rec(1000, "40M", 40, flag=0x500, mapq=0, rnext="chr2"), _rec(1000, "40M", 40, flag=0x500),
             _rec(1001, "40M", 40), _rec(1000, "40M", 40, flag=0x100, rnext="chr2"), _rec(1000, "40M", 40, rnext="chr2"),
             _rec(1002, "40M", 40, flag=0x10)]
    kept, reasons = PR.prepare(reads, 900, 1300)
    assert reasons == [PR.MAPQ, PR.DUPLICATE, PR.KEPT, PR.SECONDARY, PR.MATE_CONTIG, PR.KEPT]
    assert [k.POS for k in kept] == [1002, 1003]


def test_reverse_back_clip_extends_the_interval_and_forward_back_clip_trims():
    r = _rec(1000, "30M10S", 40, flag=0x10)
    PR.revert_soft_clipped_bases(r)
    assert PR.cigar_text(r.CIGAR) == "30M10M" and r.SEQ == SEQ(40) and r.get_interval() == (1000, 1040)
    f = _rec(1000, "30M10S", 40)
    PR.revert_soft_clipped_bases(f)
    assert PR.cigar_text(f.CIGAR) == "30M10S" and f.SEQ == SEQ(40)[:30] and f.get_interval() == (1000, 1030)
