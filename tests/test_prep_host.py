"""CPU: csrc/prep_body.hpp compiled for the host into a stand-alone program
(tests/cpp/prep_host_main.cpp) under -fsanitize=address,undefined, on exactly
sized heap blocks, over the whole grid and the compaction windows of
prep_cases.py, record for record against the restatement. No GPU and no
preloaded library."""
import subprocess

import pytest

import prep_cases as PC


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return PC.build_host_main(tmp_path_factory.mktemp("prep_host"))


def _run(exe, tmp_path, windows, check=True):
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    fin.write_text(PC.host_input(windows))
    p = subprocess.run([exe, str(fin), str(fout)], timeout=120, capture_output=True, text=True)
    if check:
        assert p.returncode == 0, p.stderr
    return p.returncode, fout.read_text()


@pytest.mark.parametrize("which", ["grid", "compaction"])
def test_host_body_equals_restatement(exe, tmp_path, which):
    windows = dict(grid=PC.grid, compaction=PC.compaction)[which]()
    _, text = _run(exe, tmp_path, windows)
    PC.assert_same(PC.parse_host_output(text), PC.expected(which), which)


def test_grid_reaches_every_outcome():
    """The grid is worth its name: every drop reason, both rewrites, front clips,
    back clips, the unsigned wrap that keeps a read whole, and empty views."""
    recs = [(r, e) for w, x in zip(PC.grid(), PC.expected("grid")) for r, e in zip(w["reads"], x["records"])]
    assert {e["drop_reason"] for _, e in recs} == {0, 1, 2, 3, 4, 5}
    assert any(e["front_to_M"] for _, e in recs) and any(e["back_to_M"] for _, e in recs)
    assert any(e["keep"] and e["offset"] and e["length"] < r["seq_len"] for r, e in recs)
    assert any(e["keep"] and e["offset"] == 0 and e["length"] < r["seq_len"] for r, e in recs)
    assert any(e["keep"] and e["end"] > PC.WIN[1] + r["seq_len"] and e["length"] == r["seq_len"] for r, e in recs)
    assert any(e["length"] == 0 for _, e in recs)
    assert {e["length"] for _, e in recs} >= {9, 10}


@pytest.mark.parametrize("defect,code", [(dict(pos=0), 1), (dict(cigar=""), 2), (dict(cigar="39M"), 4)])
def test_host_body_reports_input_errors(exe, tmp_path, defect, code):
    good = PC.read("40M", 1100)
    bad = dict(good, **defect)
    rc, text = _run(exe, tmp_path, [dict(begin=1000, end=1400, reads=[good, bad])], check=False)
    assert rc == 3 and text.split() == ["E", "0", "1", str(code)]
    # the same defect behind a flag filter is never looked at
    rc, text = _run(exe, tmp_path, [dict(begin=1000, end=1400, reads=[good, dict(bad, mapq=5)])])
    assert PC.parse_host_output(text)[0]["records"][1]["drop_reason"] == 1
