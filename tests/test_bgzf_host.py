"""CPU: csrc/bgzf_body.hpp compiled for the host into a stand-alone program
(tests/cpp/bgzf_host_main.cpp) under -fsanitize=address,undefined, the file,
every member's DEFLATE stream and every member's output in heap blocks of
exactly their sizes: every well-formed file of bam_cases.bgzf_cases() inflates
to what zlib.decompress gives, member table included, and every malformed file
of bam_cases.malformed_cases() ends with its error code at its member. Then the
streams that zlib never writes (what they exercise is asserted in
test_bgzf_census.py): written_file(), alignment_file() and the libdeflate
fixture's members as one file, compared member by member;
written_malformed_cases(); and 2 000 seeded mutants of small streams in one run
of the program's batch mode, with zlib's verdict as the expected one. No GPU and
no preloaded library."""
import os
import subprocess
import zlib

import pytest

import bam_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("bgzf_host") / "bgzf_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DBGZF_HOST_ONLY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "bgzf_host_main.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, tmp_path, file):
    fin, fout = tmp_path / "in.bgzf", tmp_path / "out.bin"
    fin.write_bytes(file)
    p = subprocess.run([exe, str(fin), str(fout)], timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [r.split() for r in p.stdout.splitlines()]
    return fout.read_bytes(), [tuple(int(x) for x in r[1:]) for r in rows if r[0] == "M"], rows[-1]


def test_the_set_has_stored_fixed_and_dynamic_blocks():
    """On the expected side, so that the set cannot hide a failure."""
    kinds = {name: {BC.first_block_type(s) for _, s, _, n in BC.members(file) if n}     # the end-of-file member left out
             for name, (file, _) in BC.bgzf_cases().items()}
    assert kinds["level_0"] == {0} and kinds["fixed"] == {1} and kinds["level_6"] == {2} and kinds["mixed_300"] == {0, 1, 2}
    assert kinds["stored_then_dynamic"] == {0} and kinds["mem_level_1"] == {2}
    sizes = {name: [n for _, _, _, n in BC.members(file)] for name, (file, _) in BC.bgzf_cases().items()}
    assert sizes["isize_0_then_data"][0] == 0 and sizes["isize_1"][0] == 1 and sizes["isize_65280"][0] == 65280
    assert sizes["isize_65536"][0] == 65536 and len(sizes["mixed_300"]) == 301
    assert len(BC.members(BC.bgzf_cases()["no_eof_marker"][0])[-1][1]) > 2


@pytest.mark.parametrize("name", sorted(BC.bgzf_cases()))
def test_well_formed_files_inflate_to_zlibs_bytes(exe, tmp_path, name):
    file, want = BC.bgzf_cases()[name]
    got, table, last = _run(exe, tmp_path, file)
    assert last == ["OK"]
    assert got == want
    off, exp = 0, []
    for k, (coff, _, _, isize) in enumerate(BC.members(file)):
        exp.append((k, coff, off, isize))
        off += isize
    assert table == exp


@pytest.mark.parametrize("name", sorted(BC.malformed_cases()))
def test_malformed_files_end_with_their_error(exe, tmp_path, name):
    file, at, code = BC.malformed_cases()[name]
    got, table, last = _run(exe, tmp_path, file)
    assert last[0] == "E" and (int(last[1]), int(last[2])) == (at, code), last
    assert len(table) == at


def _by_member(got, table, file, names):
    """Bytes and table against zlib's, member by member, so that a failure names its case."""
    off = 0
    for k, ((coff, stream, _, isize), name) in enumerate(zip(BC.members(file), names)):
        assert k < len(table), f"no member {k} ({name})"
        assert table[k] == (k, coff, off, isize), name
        assert got[off:off + isize] == zlib.decompress(stream, -15), f"member {k} ({name})"
        off += isize


def _files():
    lib = BC.libdeflate_members()
    return dict(written=(BC.written_file(), BC.written_names() + ["eof"]),
                alignment=(BC.alignment_file(), [f"member {k}" for k in range(200)]),
                libdeflate=(BC.file_of((s, d) for _, s, d in lib), [n for n, _, _ in lib] + ["eof"]))


@pytest.mark.parametrize("which", ["written", "alignment", "libdeflate"])
def test_streams_zlib_never_writes(exe, tmp_path, which):
    (file, want), names = _files()[which]
    got, table, last = _run(exe, tmp_path, file)
    _by_member(got, table, file, names)
    assert last == ["OK"] and got == want and len(table) == len(BC.members(file))


@pytest.mark.parametrize("name", sorted(BC.written_malformed_cases()))
def test_written_malformed_files_end_with_their_error(exe, tmp_path, name):
    file, at, code = BC.written_malformed_cases()[name]
    got, table, last = _run(exe, tmp_path, file)
    assert last[0] == "E" and (int(last[1]), int(last[2]), int(last[3])) == (at, code, BC.malformed_offset(at)), last
    assert len(table) == at and got == zlib.decompress(BC.members(file)[0][1], -15)


def test_mutants_get_zlibs_verdict(exe, tmp_path):
    """2 000 mutants, a file each, in one run of the program: what zlib accepts inflates to zlib's bytes, what
    zlib refuses ends with an error of the stream (any code but CRC32's)."""
    ms = BC.mutants(2000, 1)
    for k, (stream, data) in enumerate(ms):
        (tmp_path / f"{k}.bgzf").write_bytes(BC.mutant_member(stream, data) + BC.EOF_MARKER)
    p = subprocess.run([exe, "--batch", str(tmp_path), str(len(ms))], timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [r.split() for r in p.stdout.splitlines()]
    assert len(rows) == len(ms)
    for k, ((stream, data), row) in enumerate(zip(ms, rows)):
        got = (tmp_path / f"{k}.bin").read_bytes()
        if data is None:
            assert row[0] == "E" and int(row[1]) == 0 and int(row[2]) not in (0, BC.ERR_CRC), (k, row, stream.hex())
            assert int(row[2]) in (BC.ERR_STREAM, BC.ERR_EARLY, BC.ERR_DISTANCE, BC.ERR_COUNT) and got == b""
            # ISIZE is 65 536 there: a wrong count can only be more than that, not a bad stream taken for a good one
            assert int(row[2]) != BC.ERR_COUNT or BC.zlib_overflows(stream), (k, row, stream.hex())
        else:
            assert row == ["OK"] and got == data, (k, row, stream.hex())
