"""CPU: csrc/interval_body.hpp and csrc/interval_host.hpp compiled for the host
into a stand-alone program (tests/cpp/intervals_host_main.cpp) under
-fsanitize=address,undefined, every table in a heap block of exactly its size:
the program checks and merges an interval list and then decides `asked` per
window and the scope per record as interval_ask_kernel and
interval_scope_kernel do. The test compares with the restatement of
intervals_restate.py, which has no binary search and none of the body's
arithmetic. Merges of unsorted, nested, abutting and duplicate intervals on
interleaved contigs; region 5 with padding 0, 2 and 5 and region 245 with
padding 85 on contigs of 1, region, region + 1 and 3 * region - 1 bases, with a
one-base interval at every position (region 5) or at every position next to a
border (region 245) and every position of every contig as a read's begin; the
argument errors one at a time. No GPU and no preloaded library."""
import os
import subprocess

import pytest

import intervals_restate as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("intervals_host") / "intervals_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSAMX_HOST_ONLY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "intervals_host_main.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, tmp_path, cases):
    """cases: [(region, padding, ref_lens, intervals, records)]; per case None (the check failed at "bad") or a dict."""
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    text = []
    for region, padding, ref_lens, intervals, records in cases:
        text.append(f"{region} {padding} {len(ref_lens)} {len(intervals)} {len(records)}")
        text.append(" ".join(str(n) for n in ref_lens))
        text += [f"{c} {b} {e}" for c, b, e in intervals]
        text += [f"{c} {p}" for c, p in records]
    fin.write_text("\n".join(text) + "\n")
    p = subprocess.run([exe, str(fin), str(fout)], timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = fout.read_text().split("\n")
    at, out = 0, []
    for region, padding, ref_lens, intervals, records in cases:
        tag, n = rows[at].split()
        at += 1
        if tag == "E":
            out.append(dict(bad=int(n)))
            continue
        assert tag == "M"
        merged = [tuple(int(x) for x in r.split()) for r in rows[at:at + int(n)]]
        at += int(n)
        tag, n = rows[at].split()
        assert tag == "A"
        asked = [int(x) for x in rows[at + 1:at + 1 + int(n)]]
        at += 1 + int(n)
        assert rows[at] == "S"
        scope = [int(x) for x in rows[at + 1:at + 1 + len(records)]]
        at += 1 + len(records)
        assert rows[at] == "W"
        placed = [(c, p) for c, p in records if c >= 0 and p != 0 and p - 1 < ref_lens[c]]
        held = [[int(x) for x in r.split()] for r in rows[at + 1:at + 1 + len(placed)]]
        at += 1 + len(placed)
        assert all(h[0] == len(h) - 1 for h in held)
        out.append(dict(bad=None, merged=merged, asked=asked, scope=scope, held=[h[1:] for h in held]))
    assert rows[at:] == [""]
    return out


def _expect(region, padding, ref_lens, intervals, records):
    bad = IR.check(intervals, ref_lens)
    if bad is not None:
        return dict(bad=bad)
    asked = IR.asked(intervals, ref_lens, region, padding)
    placed = [(c, p) for c, p in records if c >= 0 and p != 0 and p - 1 < ref_lens[c]]
    return dict(bad=None, merged=IR.merge(intervals), asked=asked,
                scope=[int(IR.in_scope(c, p, ref_lens, region, padding, set(asked))) for c, p in records],
                held=[IR.windows_of(p - 1, ref_lens[c], region, padding) for c, p in placed])


MERGES = {
    "unsorted": [(0, 30, 40), (0, 5, 10), (0, 20, 25)],
    "nested": [(0, 5, 40), (0, 10, 20), (0, 39, 40), (0, 5, 6)],
    "abutting": [(0, 10, 20), (0, 20, 30), (0, 0, 10), (0, 31, 32)],
    "duplicate": [(0, 7, 9), (0, 7, 9), (0, 7, 9)],
    "overlapping_chain": [(0, 0, 3), (0, 2, 5), (0, 4, 7), (0, 8, 9)],
    "interleaved_contigs": [(2, 3, 9), (0, 1, 2), (1, 0, 50), (2, 0, 4), (0, 2, 3), (1, 49, 50), (2, 20, 21), (0, 0, 1)],
    "one_contig_of_three": [(1, 10, 11)],
}


@pytest.mark.parametrize("name", sorted(MERGES))
def test_merge_equals_the_maximal_runs(exe, tmp_path, name):
    ref_lens = [40, 50, 21]
    iv = MERGES[name]
    records = [(c, p) for c in range(3) for p in range(0, ref_lens[c] + 2)] + [(-1, 1)]
    got, = _run(exe, tmp_path, [(5, 2, ref_lens, iv, records)])
    exp = _expect(5, 2, ref_lens, iv, records)
    assert got == exp
    assert got["merged"] == IR.merge_sorted(iv) and got["merged"] == sorted(got["merged"])
    assert 0 < sum(got["scope"]) < len(records)


def _near_borders(n, region, padding):
    near = set()
    for b in range(0, n + region, region):
        for d in (-padding - 1, -padding, -padding + 1, -1, 0, 1, padding - 1, padding, padding + 1):
            near.add(b + d)
    return sorted(p for p in near | {0, n - 1} if 0 <= p < n)


@pytest.mark.parametrize("region,padding", [(5, 0), (5, 2), (5, 5), (245, 85)])
def test_asked_windows_and_scope_of_one_base_intervals(exe, tmp_path, region, padding):
    ref_lens = [1, region, region + 1, 3 * region - 1]
    records = [(c, p) for c, n in enumerate(ref_lens) for p in range(0, n + 2)] + [(-1, 1), (-1, 0)]
    cases = []
    for c, n in enumerate(ref_lens):
        for p in (range(n) if region == 5 else _near_borders(n, region, padding)):
            cases.append((region, padding, ref_lens, [(c, p, p + 1)], records))
    got = _run(exe, tmp_path, cases)
    first = [0]
    for n in ref_lens:
        first.append(first[-1] + -(-n // region))
    assert first[-1] == 1 + 1 + 2 + 3
    asked_of, depths = set(), set()
    for case, g in zip(cases, got):
        e = _expect(*case)
        assert g == e, case[3]
        (c, p, _), = case[3]
        assert g["asked"] == [first[c] + p // region]                     # one base asks its own window and no other
        asked_of.add((c, p // region))
        depths |= {len(h) for h in g["held"]}
    # window 0's unpadded front and the last window cut at the contig's end were asked
    assert (3, 0) in asked_of and (3, 2) in asked_of and (0, 0) in asked_of
    assert depths == {1} | ({2} if padding else set()) | ({3} if padding == region else set())


def test_a_position_is_held_by_the_windows_its_padding_reaches(exe, tmp_path):
    ref_lens = [3 * 5 - 1]
    records = [(0, p + 1) for p in range(ref_lens[0])]
    (a, b, c) = _run(exe, tmp_path, [(5, pad, ref_lens, [(0, 0, 1)], records) for pad in (0, 2, 5)])
    assert a["held"] == [[p // 5] for p in range(14)]
    assert b["held"][:8] == [[0], [0], [0], [0, 1], [0, 1], [0, 1], [0, 1], [1]]       # window 0: [0, 7), window 1: [3, 12)
    assert c["held"][4:6] == [[0, 1], [0, 1, 2]] and c["held"][9:11] == [[0, 1, 2], [1, 2]]
    assert a["scope"] == [1] * 5 + [0] * 9 and b["scope"] == [1] * 7 + [0] * 7 and c["scope"] == [1] * 10 + [0] * 4


@pytest.mark.parametrize("iv,bad", [([(0, 0, 5), (3, 0, 1)], 1), ([(-1, 0, 1)], 0), ([(0, -1, 3)], 0), ([(0, 3, 3)], 0),
                                    ([(0, 4, 3)], 0), ([(0, 0, 5), (1, 0, 1), (1, 0, 8)], 2), ([(2, 6, 7), (0, 5, 6)], 1)])
def test_intervals_that_are_no_range_of_their_contig(exe, tmp_path, iv, bad):
    ref_lens = [5, 7, 7]
    got, = _run(exe, tmp_path, [(5, 2, ref_lens, iv, [])])
    assert got == dict(bad=bad) and IR.check(iv, ref_lens) == bad
    ok, = _run(exe, tmp_path, [(5, 2, ref_lens, [(0, 0, 5), (1, 0, 7), (2, 6, 7)], [])])
    assert ok["bad"] is None and ok["asked"] == [0, 1, 2, 4]


# ---- csrc/bai.hpp: the index parse, reg2bins, the query and the merge -------------------------------

import struct   # noqa: E402

import bai_writer as BW   # noqa: E402

V = lambda coff, u=0: coff << 16 | u   # noqa: E731
# a record in a bin of every level; bins 4681 and 4682 meet in member 7; member 20 stands apart
EVERY_LEVEL = {0: [(V(1), V(1, 100))], 1: [(V(2), V(2, 50))], 9: [(V(3), V(3, 9))], 73: [(V(4), V(4, 7))], 585: [(V(5), V(5, 3))],
               4681: [(V(6), V(6, 10)), (V(6, 10), V(7, 5))], 4682: [(V(7, 5), V(7, 90))], 4683: [(V(20), V(21))]}
PRUNING = [V(6), V(7, 5), V(20)]          # window 0's least offset lies behind every higher-level chunk
NOT_PRUNING = [V(1), V(7, 5), V(20)]
FILE_LEN = 22


def _bai(exe, tmp_path, data, queries=(), n_ref=1, file_len=FILE_LEN):
    fi, fq, fo = tmp_path / "x.bai", tmp_path / "q.txt", tmp_path / "o.txt"
    fi.write_bytes(data)
    fq.write_text("".join(f"{r} {b} {e}\n" for r, b, e in queries))
    p = subprocess.run([exe, "bai", str(fi), str(n_ref), str(file_len), str(fq), str(fo)], timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = fo.read_text().split("\n")
    if rows[0].startswith("E "):
        assert rows[1:] == [""]
        return rows[0][2:]
    assert rows[0] == "OK"
    at, out = 1, []
    for _ in queries:
        got = {}
        for tag in "BQG":
            t, n = rows[at].split()
            assert t == tag
            got[tag] = [tuple(int(x) for x in r.split()) for r in rows[at + 1:at + 1 + int(n)]]
            at += 1 + int(n)
        out.append(got)
    assert rows[at:] == [""]
    return out


def _border_ranges():
    out = [(0, 1), (0, 2 ** 29), (2 ** 29 - 1, 2 ** 29), (2 ** 29 - 2, 2 ** 29)]
    for log2 in (14, 17, 20, 23, 26):
        b = 1 << log2
        for k in (1, 3):
            out += [(k * b - 1, k * b), (k * b, k * b + 1), (k * b - 1, k * b + 1)]      # one base each side, two bases astride
    return out


def test_reg2bins_at_every_bin_border(exe, tmp_path):
    data = BW.pack([(EVERY_LEVEL, PRUNING)])
    ranges = _border_ranges()
    got = _bai(exe, tmp_path, data, [(0, b, e) for b, e in ranges])
    for (b, e), g in zip(ranges, got):
        bins = [x for x, in g["B"]]
        assert sorted(bins) == sorted(IR.bins_of(b, e)) and len(set(bins)) == len(bins), (b, e)
        assert len(bins) == (6 if e - b == 1 else len(bins)) and BW.reg2bin(b, e) in bins
    assert len(got[1]["B"]) == 37449


@pytest.mark.parametrize("linear,name", [(PRUNING, "pruning"), (NOT_PRUNING, "not_pruning"), ([], "no_linear")])
def test_query_and_merge_equal_the_restatement(exe, tmp_path, linear, name):
    data = BW.pack([(EVERY_LEVEL, linear)], meta=True, no_coor=3)
    refs = IR.parse_bai(data)
    assert refs == [(EVERY_LEVEL, linear)]                               # the pseudo-bin is passed over
    queries = [(0, 0, 1), (0, 0, 16384), (0, 16383, 16385), (0, 16384, 32768), (0, 32768, 49152), (0, 40000, 2 ** 29),
               (0, 0, 2 ** 29), (0, 49152, 49153), (1, 0, 1), (0, 5, 5)]
    got = _bai(exe, tmp_path, data, queries)
    for (r, b, e), g in zip(queries, got):
        exp = IR.query(refs, r, b, e) if r == 0 and b < e else []
        assert sorted(g["Q"]) == sorted(exp), (name, b, e)
        assert g["G"] == IR.merge_chunks(exp), (name, b, e)
    first = got[1]
    higher = [c for b in (0, 1, 9, 73, 585) for c in EVERY_LEVEL[b]]
    if name == "pruning":
        assert sorted(first["Q"]) == EVERY_LEVEL[4681] and first["G"] == [(V(6), V(7, 5))]
    else:
        assert sorted(first["Q"]) == sorted(higher + EVERY_LEVEL[4681])
    # bins 4681 and 4682 are two chunks that abut, and member 7 holds the end of one and the begin of the other
    assert (V(6), V(7, 90)) in got[2]["G"] and (V(20), V(21)) in got[6]["G"] and len(got[6]["G"]) == (2 if name == "pruning" else 7)
    # chunks that do not touch but share a member
    share = BW.pack([({4681: [(V(3), V(4, 10))], 4682: [(V(4, 500), V(5, 1))], 4683: [(V(6), V(6, 9))]}, [])])
    g, = _bai(exe, tmp_path, share, [(0, 0, 2 ** 20)])
    assert g["G"] == [(V(3), V(5, 1)), (V(6), V(6, 9))] == IR.merge_chunks(g["Q"])


def test_bai_parse_errors_one_at_a_time(exe, tmp_path):
    good = BW.pack([(EVERY_LEVEL, PRUNING), ({}, [])])
    assert _bai(exe, tmp_path, good, [], n_ref=2) == []
    assert _bai(exe, tmp_path, BW.pack([(EVERY_LEVEL, PRUNING), ({}, [])], meta=True, no_coor=9), [], n_ref=2) == []

    def msg(data, **kw):
        m = _bai(exe, tmp_path, data, [], **dict(dict(n_ref=2), **kw))
        assert isinstance(m, str) and m.startswith("BAI: "), m
        return m
    assert "magic" in msg(b"BAM\x01" + good[4:]) and "magic" in msg(b"BAI\x02" + good[4:])
    assert "n_ref is 2, the BAM header has 3" in msg(good, n_ref=3)
    assert "n_ref is -1" in msg(good[:4] + struct.pack("<i", -1) + good[8:])
    one = lambda bins, linear=(): BW.pack([(bins, list(linear))])   # noqa: E731
    assert "negative count" in msg(good[:8] + struct.pack("<i", -1) + good[12:])                        # n_bin
    x = one({4681: [(V(1), V(2))]})
    assert "negative count" in msg(x[:16] + struct.pack("<i", -5) + x[20:], n_ref=1)                    # n_chunk
    assert "negative count" in msg(x[:-4] + struct.pack("<i", -1), n_ref=1)                             # n_intv
    assert "beg above end" in msg(one({4681: [(V(2), V(1))]}), n_ref=1)
    assert "at or past the file's length" in msg(one({4681: [(V(FILE_LEN), V(FILE_LEN))]}), n_ref=1)
    assert "at or past the file's length" in msg(one({4681: [(V(1), V(FILE_LEN, 0))]}), n_ref=1)
    assert "at or past the file's length" in msg(one({}, [V(FILE_LEN + 5)]), n_ref=1)
    assert _bai(exe, tmp_path, one({4681: [(V(FILE_LEN - 1), V(FILE_LEN - 1, 65535))]}, [V(FILE_LEN - 1)]), [], n_ref=1) == []
    assert "cut short" in msg(x[:16] + struct.pack("<i", 2 ** 30) + x[20:], n_ref=1)                    # a count the file cannot hold


def test_a_bai_cut_at_every_byte(exe, tmp_path):
    small = BW.pack([({4681: [(V(1), V(2))], 0: [(V(2), V(3))]}, [V(1)]), ({}, [])])
    assert _bai(exe, tmp_path, small, [], n_ref=2) == []
    for n in range(len(small)):
        m = _bai(exe, tmp_path, small[:n], [], n_ref=2)
        assert m == "BAI: cut short", (n, m)
    tailed = small + struct.pack("<Q", 4)
    for n in range(len(small), len(tailed) + 1):                   # the trailing n_no_coor is optional
        assert _bai(exe, tmp_path, tailed[:n], [], n_ref=2) == []
