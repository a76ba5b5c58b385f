"""CPU: the spread form of a lane's match window (csrc/seg_spread.hpp), which a
quad wave of the fp32 PairHMM pass keeps in LDS: one byte per group of four
columns, the group's match bits at bits 7:4. tests/cpp/seg_spread_main.cpp is
built alone under AddressSanitizer and UBSan and checked against numpy:
  - spread_nibbles over random 16-bit chunks and the edge chunks (0, all ones,
    every single bit): byte j of the result is nibble j from the top, << 4;
  - the layout [code][group / 4][lane][group % 4]: every (code, lane, group)
    has a byte of its own inside the wave's 5 120 bytes, and the 64 lanes of a
    read of one group fall into 64 different banks whatever their codes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def spread(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seg_spread") / "seg_spread_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "seg_spread_main.cpp"),
                    "-o", str(exe)], check=True)

    def run(chunks):
        p = subprocess.run([str(exe)], input="".join(f"{int(h):x}\n" for h in chunks), timeout=60,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.split("\n")
        words = np.array([int(x, 16) for x in lines[:len(chunks)]], np.uint64)
        groups = [int(x.split()[2]) for x in lines[len(chunks):] if x.startswith("group")]
        last = [x for x in lines if x.startswith("last")][0].split()
        return words, groups, (int(last[1]), int(last[3]))
    return run


def numpy_spread(h):
    h = np.asarray(h, np.uint64)
    out = np.zeros_like(h)
    for j in range(4):
        nib = (h >> np.uint64(12 - 4 * j)) & np.uint64(15)
        out |= (nib << np.uint64(4)) << np.uint64(8 * j)
    return out


def test_spread_nibbles_against_numpy(spread):
    rng = np.random.default_rng(13)
    chunks = np.concatenate([[0, 0xffff], 1 << np.arange(16), rng.integers(0, 1 << 16, 4000)])
    words, _, _ = spread(chunks)
    assert np.array_equal(words, numpy_spread(chunks))
    # every byte holds its pattern at bits 7:4 and nothing below
    assert not (words & np.uint64(0x0f0f0f0f)).any()


def test_layout_is_a_bijection_without_bank_conflicts(spread):
    _, goff, (last, total) = spread([0])
    assert len(goff) == 16 and total == 5 * 64 * 16 and last == total - 1
    code, lane, g = np.meshgrid(np.arange(5), np.arange(64), np.arange(16), indexing="ij")
    addr = code * 1024 + lane * 4 + np.asarray(goff)[g]
    assert len(np.unique(addr)) == addr.size and addr.min() == 0 and addr.max() == total - 1
    # little-endian order inside a spread word: group 4d + j is byte j of dword d
    assert [o % 4 for o in goff] == [j % 4 for j in range(16)]
    # a byte read of one group: 64 lanes, any codes, 64 different banks
    rng = np.random.default_rng(17)
    for gi in range(16):
        codes = rng.integers(0, 5, (200, 64))
        bank = ((codes * 1024 + np.arange(64) * 4 + goff[gi]) // 4) % 64
        assert (np.sort(bank, axis=1) == np.arange(64)).all()
