"""CPU: the restatement of the genome caller (genome_restate.py) against the
stand-in rule of include/hc_genome.h. For every contig of the fixture
(genome_cases.py) the genome result equals sam_restate run on the text filtered
by RNAME, record indices translated; then the placement errors, the FASTA
reader and the VCF over several contigs, and what the fixture promises."""
import pytest

import genome_cases as GC
import genome_restate as GR
import sam_cases as SC
import sam_restate as SR

PICKS = [("seeded", 0), ("seeded", 20261020), ("first", 0)]


@pytest.fixture(scope="module")
def g():
    return GC.genome()


def _stand_in(sam, name, ref, pick, seed, skip_unplaced=False):
    """sam_restate's contig call on the filtered text: per window (bounds, picked as whole-text indices)."""
    text, index = GR.filtered(sam, name)
    recs = SR.load_all_reads(text)["records"]
    rmap = SR.reads_map(recs, len(ref), skip_unplaced)
    picked = SR.picks(rmap, len(ref), SC.REGION, SC.PADDING, SR.pick_fn(pick, seed))
    return [(b, [index[k] for k in idx]) for b, idx in zip(SR.window_bounds(len(ref), SC.REGION, SC.PADDING), picked)], index


@pytest.mark.parametrize("pick,seed", PICKS)
def test_every_contig_equals_its_stand_in(g, pick, seed):
    r = GR.genome_windows(g["sam"], g["contigs"], pick, seed)
    assert [c["name"] for c in r["contigs"]] == list(GC.ORDER)
    assert sum(c["n_windows"] for c in r["contigs"]) == len(r["windows"]) == 76
    n_rec = 0
    for c, (name, ref) in enumerate(g["contigs"]):
        wins, index = _stand_in(g["sam"], name, ref, pick, seed)
        info = r["contigs"][c]
        assert info["n_windows"] == len(wins) and info["n_records"] == len(index), name
        assert [k for k, x in enumerate(r["contig_of"]) if x == c] == index, name
        n_rec += len(index)
        for lw, ((pb, pe, ob, oe), idx) in enumerate(wins):
            w = r["windows"][info["first_window"] + lw]
            assert (w["contig"], w["padded_begin"], w["padded_end"], w["origin_begin"], w["origin_end"], w["picked"]) == \
                (c, pb, pe, ob, oe, idx), (name, lw)
            assert w["ref_len"] == min(pe, len(ref)) - pb
    assert n_rec == len(r["contig_of"]) and -1 not in r["contig_of"]


def test_the_fixture_is_what_it_says(g):
    names = [n for n, _ in g["contigs"]]
    seen = GC.first_appearance(g["sam"])
    assert sorted(seen) == sorted(n for n in names if n != "chrEmpty") and seen != [n for n in names if n in seen]
    assert sorted(len(r) for n, r in g["contigs"] if n in GC.SHORT)[:6] == [1, 40, 64, 65, 130, 245]
    assert {1, 40, 64, 65, 245, 246} <= {len(r) for _, r in g["contigs"]}
    assert sum(len(r) for _, r in g["contigs"]) > 4 * 4096
    r = GR.genome_windows(g["sam"], g["contigs"], "first")
    recs = r["parsed"]["records"]
    text = g["sam"].decode("latin-1")
    # RNAME begins behind the first row and lies across row borders, the 255-byte one across several
    spans = []
    for k, rec in enumerate(recs):
        i = rec["line"]
        for _ in range(3):
            tok, at, i = SR.extract(text, i)
        spans.append((at - rec["line"], i - rec["line"]))
    assert any(b == 64 for b, e in spans) and any(b < 64 < e for b, e in spans) and any(b > 255 for b, e in spans)
    assert any(e - b == 255 and b // 64 != 0 and e // 64 - b // 64 >= 3 for b, e in spans)
    for name in GC.SHORT:
        c = names.index(name)
        info = r["contigs"][c]
        wins = r["windows"][info["first_window"]:info["first_window"] + info["n_windows"]]
        assert any(w["picked"] for w in wins), name
        mine = [rec["pos"] for k, rec in enumerate(recs) if r["contig_of"][k] == c]
        assert 1 in mine and len(g["contigs"][c][1]) in mine, name        # position 1 and the last position
    info = r["contigs"][names.index("chrEmpty")]
    assert info["n_records"] == 0 and info["n_windows"] == 3
    big = GC.big_table()
    assert len({n for n, _ in big}) == 300 and [x for x in big if x[0] in names] == g["contigs"]


def _with_lines(sam, at, lines):
    rows = sam.decode().split("\n")
    return "\n".join(rows[:at - 1] + lines + rows[at - 1:]).encode()


def test_placement_errors_name_the_lowest_line(g):
    names = [n for n, _ in g["contigs"]]
    base = GR.genome_windows(g["sam"], g["contigs"])
    n_alt = len(g["contigs"][names.index("chrT_alt")][1])
    cases = [dict(rname="chrNone"), dict(rname="*"), dict(rname="chrT", pos=0), dict(rname="chrT_alt", pos=n_alt + 1),
             dict(rname="chrT_al"), dict(rname="chrT_altx"), dict(rname="ch")]
    for k, kw in enumerate(cases):
        at = 20 + 7 * k
        sam = _with_lines(g["sam"], at, [SC.line(qname="bad", seq="A" * 30, **kw)])
        with pytest.raises(SR.Unplaced) as e:
            GR.genome_windows(sam, g["contigs"])
        assert e.value.line_no == at
        r = GR.genome_windows(sam, g["contigs"], skip_unplaced=True)
        # the stand-in skips it as well, or never sees it
        assert [[r["parsed"]["records"][i]["line_no"] - (r["parsed"]["records"][i]["line_no"] > at) for i in w["picked"]]
                for w in r["windows"]] == \
            [[base["parsed"]["records"][i]["line_no"] for i in w["picked"]] for w in base["windows"]], kw
    sam = _with_lines(g["sam"], 60, [SC.line(rname="chrNone"), SC.line(rname="chrU", cigar="3M")])
    sam = _with_lines(sam, 30, [SC.line(rname="chr", pos=65)])
    with pytest.raises(SR.Unplaced) as e:
        GR.genome_windows(sam, g["contigs"])
    assert e.value.line_no == 30
    sam = _with_lines(g["sam"], 60, [SC.line(rname="chrU", cigar="3M"), SC.line(rname="chrNone")])
    with pytest.raises(SR.Defective) as e:
        GR.genome_windows(sam, g["contigs"])
    assert e.value.line_no == 60
    deep = "".join(SC.line(qname=f"d{k}", rname="chrU", pos=7, mapq=0, seq="A" * 20) + "\n" for k in range(4097))
    with pytest.raises(GR.TooDeep) as e:
        GR.genome_windows((SC.HEADER + deep).encode(), g["contigs"])
    assert (e.value.contig, e.value.position) == (names.index("chrU"), 7)


def test_read_fasta():
    text = ">chrA a comment\twith tabs\nACgt\nnnAC\n>chrB\rx\nac\n\ngt\n>chrC\nA"
    assert GR.read_fasta(text) == [("chrA", "ACGTNNAC"), ("chrB", "ACGT"), ("chrC", "A")]
    assert GR.read_fasta(text.encode() + b"\n") == GR.read_fasta(text)
    assert GR.read_fasta("") == []
    for bad in (">a\n>b\nAC\n", ">a\nAC\n>b\n", ">a", "AC\n>a\nAC\n"):
        with pytest.raises(ValueError):
            GR.read_fasta(bad)


def test_vcf_over_several_contigs():
    wins = [dict(contig=0), dict(contig=0), dict(contig=1), dict(contig=2)]
    site = dict(status=0, begin=9, alleles=[b"A", b"C", b"AT"], a1=1, a2=2, genotype_quality=7)
    sites = [dict(site, region=1), dict(site, region=2, status=1), dict(site, region=3, begin=0, alleles=["G", "T"])]
    assert GR.vcf(["x", "y", "z"], wins, sites) == SR.VCF_HEADER + \
        "x\t10\t.\tA\tC,AT\t.\t.\t.\tGT:GQ\t1/2:7\n" + "z\t1\t.\tG\tT\t.\t.\t.\tGT:GQ\t1/2:7\n"
