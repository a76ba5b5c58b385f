"""GPU: hc_prep_reads (include/hc_prep.h) against the restatement
(prep_restate.py): every record field over the grid, the ordered compaction at
the wave's edges, many windows in one call against one by one, the same call
twice, and the device-side input errors."""
import ctypes as C

import numpy as np
import pytest

import hcphmm
import hcprep
import prep_cases as PC

pytestmark = pytest.mark.gpu

OP9 = 9


def test_grid_equals_restatement_on_every_field(engine):
    PC.assert_same(hcprep.prep_reads(PC.grid()), PC.expected("grid"), "grid")


def test_ordered_compaction_at_the_waves_edges(engine):
    wins, exp = PC.compaction(), PC.expected("compaction")
    assert sorted({len(w["reads"]) for w in wins}) == [0, 1, 63, 64, 65, 128, 129]
    assert any(e["kept"] == [64] for e in exp)
    assert any(e["n_kept"] == 0 and len(w["reads"]) == 129 for w, e in zip(wins, exp))
    assert any(e["n_kept"] == 129 for e in exp)
    PC.assert_same(hcprep.prep_reads(wins), exp, "compaction")


def _raw(windows):
    """Every byte the call returns."""
    p = hcprep.Prepared(windows)
    h = p.run()
    try:
        out = []
        for w in range(p.n):
            recs, kept, nk, kb = hcprep.window_arrays(h, w)
            out.append((recs.tobytes(), kept.tobytes(), nk, kb))
        return out
    finally:
        p.free(h)


def test_batched_equals_one_by_one_and_is_repeatable(engine):
    wins = PC.compaction() + PC.grid()
    together = _raw(wins)
    assert together == _raw(wins)
    for k in range(0, len(wins), 3):   # a third of them alone is enough to show independence
        assert _raw([wins[k]]) == [together[k]], k


def _bad(kind, **over):
    good = PC.read("40M", 1100)
    r = dict(pos=dict(good, pos=0), nocigar=dict(good, cigar="*"),
             op=dict(good, cigar=np.array([20 << 4, 5 << 4 | OP9, 20 << 4], np.uint32)),
             length=dict(good, cigar="39M"))[kind]
    return dict(r, **over)


@pytest.mark.parametrize("kind,text", [("pos", "pos == 0"), ("nocigar", "n_cigar == 0"), ("op", "op code"),
                                       ("length", "seq_len")])
def test_device_input_errors_name_the_lowest_read(engine, kind, text):
    good = PC.read("40M", 1100)
    filtered = [_bad(kind, mapq=5), _bad(kind, flag=0x400), _bad(kind, flag=0x100), _bad(kind, mate_same=0)]
    w0 = dict(begin=1000, end=1400, reads=[good] * 70 + filtered)
    # behind a flag filter the defect is never looked at
    ok = hcprep.prep_reads([w0])
    assert [r["drop_reason"] for r in ok[0]["records"][70:]] == [1, 2, 3, 4] and ok[0]["n_kept"] == 70
    # two offenders in window 1 (reads 3 and 66, in different rounds of the wave), one more in window 2
    w1 = dict(begin=1000, end=1400, reads=[good] * 3 + [_bad(kind)] + [good] * 62 + [_bad(kind)] + filtered)
    w2 = dict(begin=1000, end=1400, reads=[_bad(kind)])
    with pytest.raises(hcprep.PrepError) as e:
        hcprep.prep_reads([w0, w1, w2])
    assert e.value.code == hcphmm.EINVAL
    assert "window 1 read 3:" in e.value.msg and text in e.value.msg
    # the next call is correct
    PC.assert_same(hcprep.prep_reads(PC.compaction()[:8]), PC.expected("compaction")[:8], "after error")


def test_host_side_einval_and_empty_call(engine):
    L = hcprep.lib()
    h = C.c_void_p()
    assert L.hc_prep_reads(None, 0, C.byref(h)) == 0 and h.value
    assert L.hc_prep_result_window(h, 0, None, None, None, None, None) == hcphmm.EINVAL
    assert L.hc_prep_result_free(h) == 0
    with pytest.raises(hcprep.PrepError) as e:
        hcprep.prep_reads([dict(begin=10, end=9, reads=[])])
    assert e.value.code == hcphmm.EINVAL
    # windows without reads among others
    got = hcprep.prep_reads([dict(begin=0, end=10, reads=[]), PC.grid()[0], dict(begin=0, end=10, reads=[])])
    assert got[0]["n_kept"] == 0 and got[2]["records"] == []
    PC.assert_same(got[1:2], PC.expected("grid")[:1], "between empty windows")
