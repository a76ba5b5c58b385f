"""GPU: hc_sam_parse (include/hc_sam.h) against the restatement (sam_restate.py):
records, CIGAR pool, SEQ and QUAL bytes through the views and defect codes over
the grid of sam_cases.py; a text that goes up in many staging pieces; every
error text names the lowest line and the field and leaves the engine usable;
the same call twice gives the same bytes; the exports."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hccontig
import hcphmm
import sam_cases as SC
import sam_restate as SR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(SC.texts()))
def test_parse_equals_restatement(engine, name):
    text = SC.texts()[name]
    got, exp = hccontig.parse_sam(text), SC.expected(name)
    SC.assert_same_parse(got, exp, name)
    # SEQ and QUAL through the views: the very bytes `>>` would have extracted
    for r in got["records"]:
        toks = text[int(r["line"]):].split(b"\n", 1)[0].split()
        assert hccontig.seq(text, r) == toks[9] and hccontig.qual(text, r) == toks[10]
    assert not got["records"]["reserved"].any()


def test_grid_reaches_every_defect(engine):
    got = hccontig.parse_sam(SC.texts()["grid"])
    assert set(got["records"]["defect"].tolist()) == {0, 1, 2, 3, 4, 5}


def test_text_in_many_staging_pieces(engine, monkeypatch):
    """4096-byte pieces: the grid goes up in some eighty, lines straddle the
    seams (a 131 KB line crosses more than thirty) and the bytes are the same."""
    text = SC.texts()["grid"]
    whole = hccontig.parse_sam(text)
    monkeypatch.setenv("HC_SAM_STAGE_BYTES", "4096")
    pieces = hccontig.parse_sam(text)
    starts = [int(r["line"]) for r in whole["records"]]
    assert len(text) > 20 * 4096 and any(a // 4096 != (b - 1) // 4096 for a, b in zip(starts, starts[1:]))
    for k in ("records", "line_no", "pool"):
        assert pieces[k].tobytes() == whole[k].tobytes(), k
    SC.assert_same_parse(pieces, SC.expected("grid"), "pieces")


def test_same_call_twice_gives_the_same_bytes(engine):
    a, b = (hccontig.parse_sam(SC.texts()["grid_crlf"]) for _ in range(2))
    for k in ("records", "line_no", "pool"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_syntax_errors_name_the_lowest_line_and_the_field(engine):
    for name, text, line_no, field in SC.error_texts():
        with pytest.raises(hccontig.ContigError) as e:
            hccontig.parse_sam(text)
        assert e.value.code == hcphmm.EINVAL, name
        assert e.value.msg.startswith(f"line {line_no}: ") and SC.ERROR_TEXT[field] in e.value.msg, (name, e.value.msg)
    # the engine parses a good text afterwards
    SC.assert_same_parse(hccontig.parse_sam(SC.texts()["no_header"]), SC.expected("no_header"), "after errors")


def test_argument_errors_and_empty_text(engine):
    L = hccontig.lib()
    h = C.c_void_p()
    assert L.hc_sam_parse(None, 0, C.byref(h)) == 0 and h.value
    n = C.c_int32(-1)
    assert L.hc_sam_result_records(h, None, None, C.byref(n), None, None, None) == 0 and n.value == 0
    assert L.hc_sam_result_free(h) == 0
    assert L.hc_sam_parse(None, 5, C.byref(h)) == hcphmm.EINVAL
    assert L.hc_sam_parse(b"x", -1, C.byref(h)) == hcphmm.EINVAL
    assert L.hc_sam_parse(b"x", 1, None) == hcphmm.EINVAL
    assert L.hc_sam_result_records(None, None, None, None, None, None, None) == hcphmm.EINVAL
    assert L.hc_sam_result_free(None) == 0


def test_exports_and_mirrors_every_declared_symbol(engine):
    sam = hccontig.declared_symbols(hccontig.HEADER_SAM)
    assert sam == ["hc_sam_parse", "hc_sam_result_free", "hc_sam_result_records"]
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [s for s in sam if s not in exported]
    assert [s for s in hccontig.mirrored_symbols() if s.startswith("hc_sam_")] == sam
    assert C.sizeof(hccontig.Record) == hccontig.RECORD_DTYPE.itemsize == 48
