"""GPU: hc_bgzf_inflate (include/hc_bam.h) through hcbam.inflate against
zlib.decompress, byte for byte, on the files of bam_cases.bgzf_cases(): members
of ISIZE 0, 1, 65 280 and 65 536, stored, fixed and dynamic blocks (level 0,
Z_FIXED, levels 1, 6 and 9), many dynamic blocks in one member (mem_level 1), an
empty stored block (Z_FULL_FLUSH), a run of one byte, a second half that repeats
the first at distance 32 768, random bytes and 300 members of mixed kinds. The
malformed files of bam_cases.malformed_cases() (the same that test_bgzf_host.py
runs through the host build of the inflater under the sanitizers) each in a
child process of its own, under a time limit: HC_PHMM_EINVAL naming the member,
and a well-formed call that still succeeds behind it."""
import json
import os
import subprocess
import sys

import pytest

import bam_cases as BC
import hcbam
import hcphmm

pytestmark = pytest.mark.gpu


def test_the_set_has_stored_fixed_and_dynamic_blocks():
    """On the expected side, so that the set cannot hide a failure."""
    kinds = set()
    for file, _ in BC.bgzf_cases().values():
        kinds |= {BC.first_block_type(s) for _, s, _, n in BC.members(file) if n}
    assert kinds == {0, 1, 2}
    sizes = {n for file, _ in BC.bgzf_cases().values() for _, _, _, n in BC.members(file)}
    assert {0, 1, 65280, 65536} <= sizes


@pytest.mark.parametrize("name", sorted(BC.bgzf_cases()))
def test_inflate_equals_zlib(engine, name):
    file, want = BC.bgzf_cases()[name]
    got = hcbam.inflate(file)
    assert len(got["bytes"]) == len(want)
    assert got["bytes"] == want
    ms = BC.members(file)
    assert got["compressed_offset"] == [m[0] for m in ms] and got["isize"] == [m[3] for m in ms]
    off = 0
    for k, m in enumerate(ms):
        assert got["inflated_offset"][k] == off
        off += m[3]


def test_empty_input_and_two_runs(engine):
    assert hcbam.inflate(b"") == dict(bytes=b"", compressed_offset=[], inflated_offset=[], isize=[])
    file, _ = BC.bgzf_cases()["mixed_300"]
    assert hcbam.inflate(file) == hcbam.inflate(file)


_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import bam_cases as BC, hcbam, hcphmm
hcphmm.ensure_built(); hcphmm.init(0)
file, at, code = BC.malformed_cases()[{name!r}]
try:
    hcbam.inflate(file)
    out = dict(code=0, msg="")
except hcbam.BamError as e:
    out = dict(code=e.code, msg=e.msg)
good, want = BC.bgzf_cases()["level_6"]
out["after"] = hcbam.inflate(good)["bytes"] == want
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("name", sorted(BC.malformed_cases()))
def test_malformed_member_is_named_and_the_engine_lives(engine, name):
    file, at, code = BC.malformed_cases()[name]
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=[here, os.path.dirname(hcbam.__file__)], name=name)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["code"] == hcphmm.EINVAL, out
    assert out["msg"].startswith(f"member {at} at offset {BC.malformed_offset(at)}: "), out
    assert out["after"] is True
