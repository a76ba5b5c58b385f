"""CPU: csrc/sam_body.hpp compiled for the host into a stand-alone program
(tests/cpp/sam_host_main.cpp) under -fsanitize=address,undefined, the text in a
heap block of exactly its length, over the whole grid and every error text of
sam_cases.py, record for record and word for word against the restatement. No
GPU and no preloaded library."""
import subprocess

import pytest

import sam_cases as SC


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return SC.build_host_main(tmp_path_factory.mktemp("sam_host"))


def _run(exe, tmp_path, text):
    fin, fout = tmp_path / "in.sam", tmp_path / "out.txt"
    fin.write_bytes(text)
    p = subprocess.run([exe, str(fin), str(fout)], timeout=120, capture_output=True, text=True)
    return p, fout.read_text()


@pytest.mark.parametrize("name", sorted(SC.texts()))
def test_host_body_equals_restatement(exe, tmp_path, name):
    p, out = _run(exe, tmp_path, SC.texts()[name])
    assert p.returncode == 0, p.stderr
    SC.assert_same_parse(SC.parse_host_output(out), SC.expected(name), name)


def test_host_body_names_the_lowest_line_and_the_field(exe, tmp_path):
    for name, text, line_no, field in SC.error_texts():
        p, out = _run(exe, tmp_path, text)
        assert p.returncode == 3, (name, p.returncode, p.stderr)
        tok = out.split()
        assert tok[0] == "E" and int(tok[1]) == line_no and SC.ERROR_CODES[int(tok[2])] == field, (name, out)
