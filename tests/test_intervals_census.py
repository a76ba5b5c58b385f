"""CPU: what the files of the indexed interval call's GPU tests exercise, stated
here so that a claim about an input cannot go stale: the member counts of the
sorted twelve-contig genome, that every contig there is shorter than 16 KiB (so
that index can only choose by reference), and that on the designed big-contig
file the restated query of intervals_restate.py reads fewer than half of the
file's members for every interval set the GPU test uses. No GPU and no library."""
import pytest

import bai_writer as BW
import bam_cases as BC
import intervals_cases as IC
import intervals_restate as IR


@pytest.mark.parametrize("member_size,members", [(4096, 352), (1024, 1404), (65280, 24)])
def test_member_counts_of_the_sorted_genome(member_size, members):
    f = IC.sorted_genome(member_size)
    assert len(BC.members(f["bam"])) == members
    assert BC.sam_of(f["bam"]) == f["sam"]


def test_the_genomes_index_can_only_choose_by_reference():
    f = IC.sorted_genome(4096)
    assert max(n for _, n in f["refs"]) < 16384
    for bins, linear in IR.parse_bai(f["bai"]):
        assert set(bins) <= {4681} and len(linear) <= 1
    names = [n for n, _ in f["contigs"]]
    chosen, header, every = IC.restated_members(f, IC.by_name(names, ("chrU", 150, 151)))
    assert 0 < len(chosen) < len(every) // 4 and len(header) == 1


@pytest.mark.parametrize("name", sorted(IC.BIG_SETS))
def test_the_big_contigs_query_reads_fewer_than_half_of_the_members(name):
    f = IC.big_contig()
    chosen, header, every = IC.restated_members(f, IC.BIG_SETS[name])
    assert 0 < len(chosen) + len(header) < len(every) / 2, (len(chosen), len(header), len(every))
    assert len(header) == 1 and len(every) > 40


def test_the_big_contigs_index_has_bins_of_three_levels_and_a_full_linear_index():
    f = IC.big_contig()
    (bins, linear), = IR.parse_bai(f["bai"])
    # astride 16 384: the first 2^17-bin; astride 131 072 and 262 144: the first 2^20-bin, twice
    assert len(bins[585]) == 1 and len(bins[73]) == 2 and not [b for b in bins if b < 4681 and b not in (73, 585)]
    assert len([b for b in bins if b >= 4681]) == 8                # one 16 KiB bin per cluster
    assert len(linear) == (IC.CLUSTERS[-1] + 40 * 3 + 60) // 16384 + 1 and sorted(linear) == linear and linear[0] > 0
    mem, _, _, recs = BW.layout(f["bam"])
    assert len(recs) == 8 * 40 + 3
