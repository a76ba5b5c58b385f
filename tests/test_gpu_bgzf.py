"""GPU: hc_bgzf_inflate (include/hc_bam.h) through hcbam.inflate against
zlib.decompress, byte for byte, on the files of bam_cases.bgzf_cases(): members
of ISIZE 0, 1, 65 280 and 65 536, stored, fixed and dynamic blocks (level 0,
Z_FIXED, levels 1, 6 and 9), many dynamic blocks in one member (mem_level 1), an
empty stored block (Z_FULL_FLUSH), a run of one byte, a second half that repeats
the first (32 768 bytes back, which zlib's window cannot reach: its matches stop
near 32 500; distance 32 768 itself comes from deep15 and every_code_* below),
random bytes and 300 members of mixed kinds. The malformed files of
bam_cases.malformed_cases() (the same that test_bgzf_host.py runs through the
host build of the inflater under the sanitizers) each in a child process of its
own, under a time limit: HC_PHMM_EINVAL naming the member, and a well-formed
call that still succeeds behind it.

Then the streams that zlib never writes, all of which test_bgzf_host.py runs
through the host build too and whose features test_bgzf_census.py asserts:
written_file() (code lengths up to 15, HCLEN 19, runs across the two alphabets,
0 and 1 distance codes, every length and distance symbol at both ends of its
extra bits, distance 32 768, overlapping copies at distances that do and do not
divide 64, 1 504 blocks in one member, a member that ends on a match at 65 536),
alignment_file() (every out_off & 15 against the small ISIZEs, for the 16-byte
copy-out and the CRC32's slices), the libdeflate fixture and 390 mutants that
zlib accepts, each as one call compared member by member; and
written_malformed_cases() and 64 mutants that zlib refuses, in groups, a child
process per group."""
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


# ---- streams that zlib never writes (what they exercise: test_bgzf_census.py) -------------------------

def _equal_by_member(got, file, want, names):
    ms = BC.members(file)
    assert got["compressed_offset"] == [m[0] for m in ms] and got["isize"] == [m[3] for m in ms]
    off = 0
    for k, (m, name) in enumerate(zip(ms, names)):
        assert got["inflated_offset"][k] == off, name
        assert got["bytes"][off:off + m[3]] == want[off:off + m[3]], f"member {k} ({name}) at out_off & 15 = {off & 15}"
        off += m[3]
    assert len(got["bytes"]) == len(want) == off and got["bytes"] == want


def test_written_file(engine):
    file, want = BC.written_file()
    assert BC.inflate(file) == want
    _equal_by_member(hcbam.inflate(file), file, want, BC.written_names() + ["eof"])


def test_alignment_file(engine):
    file, want = BC.alignment_file()
    assert BC.inflate(file) == want
    ms = BC.members(file)
    _equal_by_member(hcbam.inflate(file), file, want, [f"isize {m[3]}" for m in ms])


def test_libdeflate_members(engine):
    lib = BC.libdeflate_members()
    file, want = BC.file_of((s, d) for _, s, d in lib)
    assert BC.inflate(file) == want and len(BC.members(file)) == 33
    _equal_by_member(hcbam.inflate(file), file, want, [n for n, _, _ in lib] + ["eof"])


def test_accepted_mutants_inflate_to_zlibs_bytes(engine):
    """The first 390 mutants of mutants(2000, 1) that zlib accepts, as the members of one file, in one call."""
    kept = [(k, s, d) for k, (s, d) in enumerate(BC.mutants(2000, 1)) if d is not None][:390]
    assert len(kept) == 390
    file, want = BC.file_of((s, d) for _, s, d in kept)
    _equal_by_member(hcbam.inflate(file), file, want, [f"mutant {k}: {s.hex()}" for k, s, _ in kept] + ["eof"])


_GROUP_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import bam_cases as BC, hcbam, hcphmm
hcphmm.ensure_built(); hcphmm.init(0)
good, want = BC.bgzf_cases()["level_6"]
prefix = "member 1 at offset %d: " % BC.malformed_offset(1)
for name, file, texts in BC.device_refusals({kind!r})[{group}]:
    try:
        hcbam.inflate(file)
        code, msg = 0, ""
    except hcbam.BamError as e:
        code, msg = e.code, e.msg
    print("RESULT " + json.dumps([name, code, msg]), flush=True)
    if code != hcphmm.EINVAL or msg not in [prefix + t for t in texts]:
        sys.exit(3)                      # not the clean refusal: no further call on the device
    if hcbam.inflate(good)["bytes"] != want:
        print("RESULT " + json.dumps([name, -1, "a good file no longer inflates"]), flush=True)
        sys.exit(4)
"""


@pytest.mark.parametrize("kind,group", [("written", g) for g in range(4)] + [("mutants", g) for g in range(4)])
def test_refusals_name_the_member_and_the_engine_lives(engine, kind, group):
    """A child process takes a group of malformed files in turn and ends at the first outcome that is not the
    expected refusal; the parent does not retry."""
    rows = BC.device_refusals(kind)[group]
    assert len(BC.device_refusals(kind)) == 4
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, "-c", _GROUP_CHILD.format(paths=[here, os.path.dirname(hcbam.__file__)], kind=kind,
                                                                  group=group)], capture_output=True, text=True, timeout=120)
    seen = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0, (seen[-1:], p.stderr[-2000:])
    assert [s[0] for s in seen] == [r[0] for r in rows]
