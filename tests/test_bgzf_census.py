"""CPU, on the expected side only (no engine, no host program): what the inputs
of the BGZF inflater's tests exercise, stated by deflate_census.walk and
asserted here, so that a claim about an input cannot go stale unnoticed. Every
census is used only after walk() returned exactly zlib.decompress(stream, -15).

The properties of bam_cases.written_cases() (streams from deflate_writer that
zlib never writes), one test per case; that zlib's own encoding of the same
bytes has none of them; the coverage of alignment_file() from its member table;
zlib's verdict on written_malformed_cases(); the two directions of mutants();
and the union over bgzf_cases(), written_cases() and the libdeflate fixture."""
import zlib

import pytest

import bam_cases as BC
import deflate_census as DC
import deflate_writer as W


def census(stream, data=None):
    want = zlib.decompress(stream, -15)
    got, c = DC.walk(stream)
    assert got == want
    assert data is None or want == data
    return c


@pytest.fixture(scope="module")
def written():
    """name -> census, after zlib.decompress gave expand(tokens) for the case."""
    return {name: census(s, d) for name, (s, d) in BC.written_cases().items()}


ALL_LENGTHS = set(range(257, 286))
ALL_DISTS = set(range(30))
BOTH = lambda symbols: {(s, e) for s in symbols for e in (0, 1)}                 # noqa: E731


def test_deep15(written):
    c = written["deep15"]
    lit, dist = BC._deep15_lens()
    assert sorted(lit.values()) == sorted(dist.values()) == list(range(1, 16)) + [15]
    assert lit[256] == lit[285] == dist[29] == 15
    assert c["blocks"] == 1 and c["lit_declared"] == c["dist_declared"] == set(range(1, 16))
    assert c["lit_used"] == c["dist_used"] == set(range(1, 16))
    assert c["length_symbols"] == {285} and {28, 29} <= c["dist_symbols"] == set(range(14, 30))   # both 15-bit codes of each
    assert c["hclen"] == {19} and c["hlit"] == {29} and c["hdist"] == {29}
    assert c["max_distance"] == 32768 and c["ends_on_match"] and (258, 32768) in c["matches"]
    stream, data = BC.written_cases()["deep15"]
    assert len(data) - 258 >= 32768 and data[-258:] == data[-258 - 32768:-32768]


@pytest.mark.parametrize("name", ["every_code_fixed", "every_code_dynamic"])
def test_every_code(written, name):
    c = written[name]
    assert c["blocks"] == 1 and c["block_types"] == ({1} if name.endswith("fixed") else {2})
    assert c["length_symbols"] == ALL_LENGTHS and c["dist_symbols"] == ALL_DISTS
    assert c["length_extremes"] == BOTH(ALL_LENGTHS) and c["dist_extremes"] == BOTH(ALL_DISTS)
    assert c["max_distance"] == 32768
    assert BC.written_cases()["every_code_fixed"][1] == BC.written_cases()["every_code_dynamic"][1]
    if name.endswith("dynamic"):
        assert c["hlit"] == {29} and c["hdist"] == {29}
        assert max(c["lit_declared"]) == max(c["dist_declared"]) == 15
        assert sorted(W.complete(286, 15)) == W.complete(286, 15) and sum(2.0 ** -v for v in W.complete(286, 15)) == 1.0


def test_overlaps(written):
    c = written["overlaps"]
    want = {(n, d) for d in list(range(1, 67)) + [127, 128, 129, 257] for n in (3, 64, 65, 258)}
    assert c["matches"] == want
    assert c["overlaps"] == {d for n, d in want if d < n} >= set(range(1, 67)) | {127, 128, 129, 257}


def test_distance_code_counts(written):
    c = written["no_distance_code"]
    assert c["hdist"] == {0} and c["dist_code_counts"] == {0} and c["dist_declared"] == set() and not c["matches"]
    c = written["one_distance_code"]
    assert c["dist_code_counts"] == {1} and c["dist_declared"] == {1} and len(c["dist_symbols"]) == 1
    assert len(c["matches"]) >= 8 and 258 in {n for n, _ in c["matches"]}
    c = written["hlit_0"]
    assert c["hlit"] == {0} and not c["matches"] and c["blocks_without_match"] == 1


def test_runs_across_the_alphabets(written):
    assert written["run_across_alphabets"]["crossing_runs"] == [16]
    assert written["zero_run_across_alphabets"]["crossing_runs"] == [18]
    for name in ("run_across_alphabets", "zero_run_across_alphabets"):
        assert written[name]["matches"]                      # the distance lengths behind the run are used


def test_tiny_blocks(written):
    c = written["tiny_blocks"]
    assert c["blocks"] >= 1500 and c["block_types"] == {0, 1, 2} and c["empty_stored"] >= 375
    assert c["last_block"] == (0, 0)
    assert c["matches_across_blocks"] >= 700
    kinds = [k for k, _ in c["block_list"]]
    assert kinds == [1, 2, 0, 0] * (len(kinds) // 4)                       # fixed, dynamic, stored, empty stored in turn
    assert all(n == 0 for _, n in c["block_list"][3::4]) and all(n == 3 for _, n in c["block_list"][2::4])
    # a fixed block begins with a match at distance 4 and more: over the empty block and the stored block's 3 bytes
    assert max(d for _, d in c["matches"]) >= 7


def test_ends_on_a_match_and_the_far_match(written):
    c = written["ends_on_a_match"]
    stream, data = BC.written_cases()["ends_on_a_match"]
    assert len(data) == 65536 and c["ends_on_match"] and c["blocks"] == 1
    assert data[-258:] == data[-1258:-1000] and (258, 1000) in c["matches"]
    assert max(c["lit_declared"]) == max(c["dist_declared"]) == 15 and c["hclen"] == {19}
    c = written["stored_then_far_match"]
    assert c["matches"] == {(258, 20000)} and c["block_types"] == {0, 1}


def test_zlibs_encoding_of_the_same_bytes_has_none_of_this(written):
    """The inputs carry the features, not merely the bytes."""
    for name, (_, data) in BC.written_cases().items():
        for level in (1, 6, 9):
            c = census(BC.deflate(data, level=level), data)
            assert max(c["lit_declared"] | c["dist_declared"] | {0}) <= 13, name
            assert not c["crossing_runs"] and c["dist_code_counts"] <= {2} and 19 not in c["hclen"], name
            assert c["max_distance"] < 32768 and 0 not in c["hlit"], name
            assert c["blocks"] < 10 and c["last_block"] != (0, 0), name
            assert c["length_extremes"] != BOTH(ALL_LENGTHS), name
    c = census(BC.deflate(BC.written_cases()["overlaps"][1], level=9))
    assert not {(n, d) for d in range(1, 67) for n in (3, 64, 65, 258)} <= c["matches"]


def test_written_file_puts_the_repeats_at_another_alignment():
    file, data = BC.written_file()
    ms, names = BC.members(file), BC.written_names()
    assert len(ms) == len(names) + 1 and ms[-1][3] == 0 and BC.inflate(file) == data
    offs, at = {}, 0
    for name, m in zip(names, ms):
        assert zlib.decompress(m[1], -15) == BC.written_cases()[name][1]
        offs.setdefault(name, []).append(at & 15)
        at += m[3]
    for name in BC.AGAIN:
        assert len(offs[name]) == 2 and offs[name][0] != offs[name][1], (name, offs[name])
    assert any(m[3] % 2 for m in ms)


def test_alignment_file_meets_every_residue():
    file, data = BC.alignment_file()
    ms = BC.members(file)
    assert BC.inflate(file) == data and 100 <= len(ms) <= 130
    seen, at = set(), 0
    for _, _, _, isize in ms:
        seen.add((at & 15, isize))
        at += isize
    assert {(r, n) for r in range(16) for n in BC.ALIGN_CLASSES} <= seen
    assert set(BC.ALIGN_STEPS) <= {n for _, n in seen}
    assert {BC.first_block_type(s) for _, s, _, n in ms if n} == {0, 1, 2}


def test_zlib_refuses_what_the_malformed_cases_say():
    cases = BC.written_malformed_cases()
    codes = [code for _, _, code in cases.values()]
    assert codes.count(BC.ERR_STREAM) == 12 and codes.count(BC.ERR_EARLY) == 8 and codes.count(BC.ERR_DISTANCE) == 1
    assert codes.count(BC.ERR_COUNT) == 4 and len(cases) == 25
    for name, (file, at, code) in cases.items():
        assert at == 1
        ms = BC.members(file)                      # the containers are sound, only the streams are not
        assert len(ms) == 4 and ms[1][0] == BC.malformed_offset(1)
        data = BC.zlib_verdict(ms[1][1])
        if code == BC.ERR_COUNT:
            assert data is not None and len(data) > ms[1][3], name
        else:
            assert data is None, name
        for k in (0, 2):
            assert zlib.crc32(zlib.decompress(ms[k][1], -15)) == ms[k][2]
    # the stream one byte nearer is a good member
    assert BC.zlib_verdict(BC.written_cases()["stored_then_far_match"][0]) is not None


def test_the_fixture_is_a_second_producer():
    ms = BC.libdeflate_members()
    inputs = BC.libdeflate_inputs()
    assert len(ms) == 4 * len(inputs) == 32
    assert {n.rsplit("_level_", 1)[1] for n, _, _ in ms} == {"1", "6", "9", "12"}
    import os
    assert os.path.getsize(BC.GOLDEN_LIBDEFLATE) < 400_000
    for name, stream, data in ms:
        if name.startswith("bam_"):
            assert data[:4] == b"BAM\x01" and len(data) == 60000       # of the genome text as it was when the file was made
        else:
            assert data == inputs[name.rsplit("_level_", 1)[0]], name   # the inputs are still what was compressed
        assert len(stream) <= 65536 - 26
        census(stream, data)


def test_mutants_test_both_directions():
    ms = BC.mutants(2000, 1)
    accepted = sum(1 for _, d in ms if d is not None)
    assert 0.2 * len(ms) <= accepted <= 0.8 * len(ms)
    assert all(40 <= len(s) <= 3000 for s in BC.mutant_seeds())
    assert BC.mutants(2000, 1) == ms and len({s for s, _ in ms}) > 1900


def test_the_union_covers_the_format(written):
    cs = list(written.values())
    for name, (file, _) in BC.bgzf_cases().items():
        if name != "mixed_300":
            cs += [census(s) for _, s, _, _ in BC.members(file)]
    cs += [census(s, d) for _, s, d in BC.libdeflate_members()]
    u = DC.merge(cs)
    assert u["block_types"] == {0, 1, 2}
    every = set(range(1, 16))
    assert u["lit_declared"] == u["lit_used"] == u["dist_declared"] == u["dist_used"] == every
    assert u["length_symbols"] == ALL_LENGTHS and u["dist_symbols"] == ALL_DISTS
    assert u["max_distance"] == 32768
    assert len(u["crossing_runs"]) >= 2 and {16, 18} <= set(u["crossing_runs"])
    assert u["dist_code_counts"] == {0, 1, 2}
    assert 19 in u["hclen"] and 0 in u["hlit"] and 0 in u["hdist"]
    assert u["empty_stored"] >= 2


def test_zlibs_window_stops_short_of_32768():
    """What second_half_repeats really has: zlib never reaches back 32 768 bytes."""
    file, _ = BC.bgzf_cases()["second_half_repeats"]
    c = DC.merge(census(s) for _, s, _, n in BC.members(file) if n)
    assert 32000 < c["max_distance"] <= 32768 - 262
