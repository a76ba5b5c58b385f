"""CPU: the C ABIs of the read preparation (include/hc_prep.h) and the window
caller (include/hc_call.h) are exported and mirrored, their headers compile as
C and as C++, argument errors are HC_PHMM_EINVAL with a message before any
device work, and without a device the calls return HC_PHMM_ENODEV."""
import ctypes as C
import os
import subprocess

import pytest

import call_cases as CC
import hccall
import hcphmm
import hcprep
import prep_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def built():
    hcphmm.ensure_built()
    return hccall.lib()


def test_exports_and_mirrors_every_declared_symbol(built):
    prep, call = hcprep.declared_symbols(), hccall.declared_symbols()
    assert prep == ["hc_prep_reads", "hc_prep_result_free", "hc_prep_result_window"]
    assert call == ["hc_call_result_free", "hc_call_result_hap", "hc_call_result_matrix", "hc_call_result_prep",
                    "hc_call_result_reads", "hc_call_result_sites", "hc_call_result_window", "hc_call_windows"]
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [s for s in prep + call if s not in exported]
    assert hcprep.mirrored_symbols() == prep and hccall.mirrored_symbols() == call


def test_structs_match_the_headers(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hc_call.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(hc_prep_read),\n'
                   '  sizeof(hc_prep_window), sizeof(hc_prep_record), sizeof(hc_call_window),\n'
                   '  offsetof(hc_prep_read, mate_same_contig), offsetof(hc_prep_record, keep),\n'
                   '  offsetof(hc_prep_record, back_to_M), offsetof(hc_call_window, bases),\n'
                   '  offsetof(hc_call_window, n_reads)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(hcprep.Read), C.sizeof(hcprep.Window), C.sizeof(hcprep.Record), C.sizeof(hccall.Window),
                   hcprep.Read.mate_same_contig.offset, hcprep.Record.keep.offset, hcprep.Record.back_to_M.offset,
                   hccall.Window.bases.offset, hccall.Window.n_reads.offset]
    assert C.sizeof(hcprep.Record) == hcprep.RECORD_DTYPE.itemsize == 32


def test_headers_compile_as_c_and_cpp(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "hc_prep.h"\n#include "hc_call.h"\n'
                   'int main(void) { hc_prep_result* p = 0; hc_call_result* c = 0;\n'
                   '  unsigned w = HC_PREP_CIGAR_WORD(101, 0);\n'
                   '  return hc_prep_reads(0, 0, &p) + hc_call_windows(0, 0, HC_CALL_WANT_L | HC_CALL_F64, &c) + (int)w == 12345; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INC, str(src)], check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", INC, str(src)], check=True)


def test_cpp_dropins_compile_and_link(built, tmp_path):
    """include/hc_prep.hpp and include/hc_call.hpp against the stand-in types of tests/cpp/call_region_dropin.cpp."""
    exe = tmp_path / "dropin"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", INC, os.path.join(ROOT, "tests", "cpp", "call_region_dropin.cpp"),
                    "-L", os.path.dirname(hcphmm.LIB_PATH), "-lhcpairhmm", "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH),
                    "-o", str(exe)], check=True)
    assert exe.exists()


def _prep_rc(windows, n=None, out=True):
    L = hcprep.lib()
    p = hcprep.Prepared(windows) if not isinstance(windows, (type(None), C.Array)) else None
    h = C.c_void_p()
    rc = L.hc_prep_reads(p.arr if p else windows, len(windows) if n is None else n, C.byref(h) if out else None)
    msg = (L.hc_phmm_last_error() or b"").decode()
    assert not h.value or rc == 0
    if h.value:
        L.hc_prep_result_free(h)
    return rc, msg


def test_prep_einval_before_any_device_work(built):
    ok = dict(begin=1000, end=1400, reads=[PC.read("40M", 1100)])
    assert _prep_rc([ok], out=False)[0] == hcphmm.EINVAL
    assert _prep_rc(None, n=1)[0] == hcphmm.EINVAL
    assert _prep_rc([ok], n=-1)[0] == hcphmm.EINVAL
    rc, msg = _prep_rc([ok, dict(begin=10, end=9, reads=[])])
    assert rc == hcphmm.EINVAL and "window 1" in msg and "padded_end" in msg
    rc, msg = _prep_rc([dict(begin=-1, end=9, reads=[])])
    assert rc == hcphmm.EINVAL and "padded_begin" in msg
    for bad in (-1, 65537):
        rc, msg = _prep_rc([dict(begin=0, end=9, reads=[PC.read("40M", 0), PC.read("40M", 0, seq_len=bad)])])
        assert rc == hcphmm.EINVAL and "window 0 read 1" in msg and "seq_len" in msg
    arr = (hcprep.Window * 1)()
    arr[0] = hcprep.Window(0, 10, None, -1)
    assert _prep_rc(arr, n=1)[0] == hcphmm.EINVAL
    arr[0] = hcprep.Window(0, 10, None, 2)
    rc, msg = _prep_rc(arr, n=1)
    assert rc == hcphmm.EINVAL and "null reads" in msg
    ra = (hcprep.Read * 1)()
    ra[0] = hcprep.Read(None, 2, 1, 40, 0, 60, 1)
    arr[0] = hcprep.Window(0, 10, ra, 1)
    rc, msg = _prep_rc(arr, n=1)
    assert rc == hcphmm.EINVAL and "null cigar" in msg
    ra[0] = hcprep.Read(None, -1, 1, 40, 0, 60, 1)
    assert _prep_rc(arr, n=1)[0] == hcphmm.EINVAL


def _call_rc(windows, n=None, flags=0, out=True):
    L = hccall.lib()
    p = hccall.Prepared(windows) if not isinstance(windows, (type(None), C.Array)) else None
    h = C.c_void_p()
    rc = L.hc_call_windows(p.arr if p else windows, len(windows) if n is None else n, flags, C.byref(h) if out else None)
    msg = (L.hc_phmm_last_error() or b"").decode()
    assert not h.value or rc == 0
    if h.value:
        L.hc_call_result_free(h)
    return rc, msg


def test_call_einval_before_any_device_work(built):
    ok = dict(ref=b"A" * 50, padded_begin=0, padded_end=50, origin_begin=10, origin_end=40, reads=[])
    assert _call_rc([ok], out=False)[0] == hcphmm.EINVAL
    assert _call_rc(None, n=1)[0] == hcphmm.EINVAL
    assert _call_rc([ok], n=-1)[0] == hcphmm.EINVAL
    rc, msg = _call_rc([ok], flags=4)
    assert rc == hcphmm.EINVAL and "flags" in msg
    rc, msg = _call_rc([ok, dict(ok, ref=None)])
    assert rc == hcphmm.EINVAL and "window 1" in msg and "null ref" in msg
    assert _call_rc([dict(ok, ref=b"")])[0] == hcphmm.EINVAL
    assert _call_rc([dict(ok, ref=b"A" * 1024)])[0] == hcphmm.EINVAL
    arr = (hccall.Window * 1)()
    arr[0] = hccall.Window(b"A" * 50, 50, 0, 50, 10, 40, None, None, None, 3)
    rc, msg = _call_rc(arr, n=1)
    assert rc == hcphmm.EINVAL and "null reads" in msg
    arr[0] = hccall.Window(b"A" * 50, 50, 0, 50, 10, 40, None, None, None, -3)
    assert _call_rc(arr, n=1)[0] == hcphmm.EINVAL
    # the preparation's own argument errors come through with its message
    rc, msg = _call_rc([dict(ok, padded_end=-5)])
    assert rc == hcphmm.EINVAL and "padded_end" in msg


def test_empty_calls_and_accessor_errors(built):
    L = hccall.lib()
    h = C.c_void_p()
    assert L.hc_prep_reads(None, 0, C.byref(h)) == 0 and h.value
    assert L.hc_prep_result_window(h, 0, None, None, None, None, None) == hcphmm.EINVAL
    assert L.hc_prep_result_free(h) == 0
    assert L.hc_prep_result_window(None, 0, None, None, None, None, None) == hcphmm.EINVAL
    assert L.hc_prep_result_free(None) == 0
    h = C.c_void_p()
    assert L.hc_call_windows(None, 0, 0, C.byref(h)) == 0 and h.value
    n = C.c_int64(-1)
    assert L.hc_call_result_sites(h, None, C.byref(n)) == 0 and n.value == 0
    assert L.hc_call_result_window(h, 0, None, None, None, None) == hcphmm.EINVAL
    assert L.hc_call_result_reads(h, 0, None, None) == hcphmm.EINVAL
    assert L.hc_call_result_free(h) == 0
    assert L.hc_call_result_sites(None, None, None) == hcphmm.EINVAL
    assert L.hc_call_result_free(None) == 0


def test_no_silent_fallback_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hcprep.PrepError) as e:
        hcprep.prep_reads(PC.grid()[:1])
    assert e.value.code == hcphmm.ENODEV
    with pytest.raises(hccall.CallError) as e:
        hccall.call_windows(CC.windows(2))
    assert e.value.code == hcphmm.ENODEV


def test_pack_cigar():
    assert hcprep.pack_cigar("10M100D10M").tolist() == [10 << 4, 100 << 4 | 2, 10 << 4]
    assert hcprep.pack_cigar("5H3S2=1X4P6N7I").tolist() == [5 << 4 | 5, 3 << 4 | 4, 2 << 4 | 7, 1 << 4 | 8, 4 << 4 | 6,
                                                            6 << 4 | 3, 7 << 4 | 1]
    assert len(hcprep.pack_cigar("*")) == 0
    for bad in ("M", "10", "10Q", "10M5", "268435456M"):
        with pytest.raises(ValueError):
            hcprep.pack_cigar(bad)
