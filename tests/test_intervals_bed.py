"""CPU: hcintervals.parse_bed, the BED reading of the interval calls' Python mirror:
the first three white-space separated columns, the lines that are skipped, and
the errors with their 1-based line. No GPU and no library."""
import pytest

import hcintervals


def test_parse_bed():
    names = ["chr1", "chr2"]
    text = "# a comment\ntrack name=x\nbrowser position chr1\n\nchr2\t5\t9\tgene\t0\t+\nchr1 0 3\n"
    assert hcintervals.parse_bed(text, names) == [(1, 5, 9), (0, 0, 3)]
    assert hcintervals.parse_bed(text.encode(), names) == [(1, 5, 9), (0, 0, 3)]
    for bad, line in (("chr1\t0\t1\nchr3\t0\t1\n", 2), ("\n\nchr1\t0\n", 3), ("chr1\tx\t1\n", 1)):
        with pytest.raises(ValueError, match=f"BED line {line}:"):
            hcintervals.parse_bed(bad, names)
