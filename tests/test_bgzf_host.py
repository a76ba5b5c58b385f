"""CPU: csrc/bgzf_body.hpp compiled for the host into a stand-alone program
(tests/cpp/bgzf_host_main.cpp) under -fsanitize=address,undefined, the file,
every member's DEFLATE stream and every member's output in heap blocks of
exactly their sizes: every well-formed file of bam_cases.bgzf_cases() inflates
to what zlib.decompress gives, member table included, and every malformed file
of bam_cases.malformed_cases() ends with its error code at its member. No GPU
and no preloaded library."""
import os
import subprocess

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
