"""CPU: csrc/genome_sort_body.hpp compiled for the host into a stand-alone
program (tests/cpp/genome_sort_host_main.cpp) under
-fsanitize=address,undefined, keys and outputs in heap blocks of exactly their
sizes: the program runs the digit, pass-count, in-tile rank, head-flag, depth
and lower-bound functions as the kernels of genome_sort_kernels.hip do, tile by
tile, and the test compares with numpy.argsort(kind="stable") and a run table
made in Python. Element counts around a wave and around a tile, key widths
around every pass border up to five passes, and key sets with all keys equal,
descending, and with the sentinel of unplaced reads mixed in. No GPU and no
preloaded library."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 2048
COUNTS = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 10000)
WIDTHS = (1, 8, 9, 16, 17, 33, 40)
MAX_READS = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("genome_sort_host") / "genome_sort_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSAMX_HOST_ONLY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "genome_sort_host_main.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, tmp_path, keys, total_len, queries):
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    fin.write_text(f"{len(keys)} {total_len} {len(queries)}\n" + "\n".join(str(int(k)) for k in keys) + "\n"
                   + "\n".join(str(int(k)) for k in queries) + "\n")
    p = subprocess.run([exe, str(fin), str(MAX_READS), str(fout)], timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = fout.read_text().split("\n")
    n = len(keys)
    tile, passes = (int(x) for x in rows[0].split()[1:])
    order = [tuple(int(x) for x in r.split()) for r in rows[1:1 + n]]
    n_runs = int(rows[1 + n].split()[1])
    runs = [tuple(int(x) for x in r.split()) for r in rows[2 + n:2 + n + n_runs]]
    at = 2 + n + n_runs
    closing, deep, q = (int(rows[at + k].split()[1]) for k in range(3))
    found = [int(x) for x in rows[at + 3:at + 3 + q]]
    return dict(tile=tile, passes=passes, order=order, runs=runs, closing=closing, deep=deep, found=found)


def _key_sets(rng, n, total_len):
    """Keys in [0, total_len]; total_len itself is the key of an unplaced read."""
    top = total_len - 1
    yield "equal", np.full(n, top // 2, np.int64)
    yield "equal_top", np.full(n, top, np.int64)
    # distinct where the width allows it, descending in any case
    yield "descending", (np.arange(n - 1, -1, -1, dtype=object) * total_len // max(n, 1)).astype(np.int64)
    mixed = rng.integers(0, total_len, n, dtype=np.int64)
    if n:
        few = rng.integers(0, total_len, max(n // 40, 1), dtype=np.int64)        # positions many elements deep
        where = rng.random(n) < 0.5
        mixed[where] = few[rng.integers(0, len(few), int(where.sum()))]
        mixed[rng.random(n) < 0.1] = total_len
    yield "sentinels_mixed", mixed
    yield "all_sentinels", np.full(n, total_len, np.int64)


@pytest.mark.parametrize("width", WIDTHS)
def test_sort_runs_and_bounds_equal_numpy(exe, tmp_path, width):
    rng = np.random.default_rng(20261021 + width)
    seen_deep = seen_runs = 0
    for total_len in sorted({1 << (width - 1), (1 << width) - 1}):
        assert total_len.bit_length() == width
        for n in COUNTS:
            for name, keys in _key_sets(rng, n, total_len):
                what = (width, total_len, n, name)
                order = np.argsort(keys, kind="stable")
                placed = keys[order][keys[order] < total_len]
                pos, first, depth = np.unique(placed, return_index=True, return_counts=True)
                queries = np.concatenate([rng.integers(0, total_len + 1, 20, dtype=np.int64), [0, total_len],
                                          pos[:50], pos[:50] + 1, np.maximum(pos[:50] - 1, 0)]).astype(np.int64)
                got = _run(exe, tmp_path, keys, total_len, queries)
                assert got["tile"] == TILE and got["passes"] == -(-width // 8), what
                assert got["order"] == list(zip(keys[order].tolist(), order.tolist())), what
                assert got["runs"] == list(zip(pos.tolist(), first.tolist())), what
                assert got["closing"] == len(placed), what
                deep = pos[depth > MAX_READS]
                assert got["deep"] == (int(deep.min()) + 1 if len(deep) else 0), what
                assert got["found"] == np.searchsorted(pos, queries, "left").tolist(), what
                seen_deep += len(deep) > 0
                seen_runs += len(pos) > 1
    assert seen_deep and (seen_runs or width == 1)      # a width of one bit has position 0 only
