"""GPU: the sorted buckets of hc_genome_call (include/hc_genome.h,
HC_GENOME_SORTED_BUCKETS) against the dense path, which is the parent's code and
the exact oracle: every field and byte must be the same. The twelve contigs of
genome_cases.py for the three picks of test_gpu_genome.py, also against the
restatement (genome_restate.py); a generated text that puts the reads of one
position into different lanes, waves, rounds and tiles; tables whose positions
need four and five passes and lie past 2^31 and 2^32; depth and error parity;
edges; the selection by flag and environment in fresh processes; two identical
runs; the C++ drop-in."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import genome_cases as GC
import genome_restate as GR
import hccontig
import hcgenome
import hcphmm
import sam_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICKS = [("seeded", 0), ("seeded", 20261020), ("first", 0)]     # those of test_gpu_genome.py
WINDOW_FIELDS = ("contig", "padded_begin", "padded_end", "origin_begin", "origin_end", "ref_len", "picked", "status",
                 "asm_status", "kmer_size", "n_haps", "reads")
TILE = 2048     # csrc/genome_sort_body.hpp, kSortTile


@pytest.fixture(scope="module")
def g():
    return GC.genome()


@pytest.fixture(scope="module")
def names(g):
    return [n for n, _ in g["contigs"]]


@pytest.fixture(scope="module")
def dense(engine, g):
    return {(pick, seed): hcgenome.call_genome(g["sam"], g["contigs"], seed=seed, pick=pick, want_site_reads=True)
            for pick, seed in PICKS}


@pytest.fixture(scope="module")
def got(engine, g):
    return {(pick, seed): hcgenome.call_genome(g["sam"], g["contigs"], seed=seed, pick=pick, want_site_reads=True,
                                               sorted_buckets=True) for pick, seed in PICKS}


def _same_bytes(x, y, f):
    if isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f
    else:
        assert x == y, (f, x, y)


def assert_same_result(a, b, tag=""):
    """Every field of two call_genome results; arrays (likelihoods among them) by their bytes."""
    assert a["vcf"] == b["vcf"], tag
    assert a["contigs"] == b["contigs"], tag
    assert len(a["windows"]) == len(b["windows"]), tag
    for k, (x, y) in enumerate(zip(a["windows"], b["windows"])):
        for f in WINDOW_FIELDS:
            assert x[f] == y[f], (tag, k, f, x[f], y[f])
    assert sorted(a["sam"]) == sorted(b["sam"]), tag
    for f in a["sam"]:
        _same_bytes(a["sam"][f], b["sam"][f], (tag, f))
    assert len(a["sites"]) == len(b["sites"]), tag
    for x, y in zip(a["sites"], b["sites"]):
        assert sorted(x) == sorted(y)
        for f in x:
            _same_bytes(x[f], y[f], (tag, f))


# ---- 1. equals the dense path and the restatement

@pytest.mark.parametrize("key", PICKS)
def test_sorted_equals_dense_and_the_restatement(got, dense, g, key):
    a, d = got[key], dense[key]
    assert len(a["windows"]) == 76 and a["vcf"].count(b"\n") > 4 + 5 and any(w["picked"] for w in a["windows"])
    assert_same_result(a, d, key)
    r = GR.genome_windows(g["sam"], g["contigs"], *key)
    assert a["sam"]["contig_of"].tolist() == r["contig_of"] and a["contigs"] == r["contigs"]
    for k, (x, y) in enumerate(zip(a["windows"], r["windows"])):
        for f in WINDOW_FIELDS[:7]:
            assert x[f] == y[f], (k, f, x[f], y[f])


# ---- 2. the order within a position across lanes, waves, rounds and tiles

def _deep_text(g):
    """10 007 reads of 20 bases with MAPQ 0 (the picks take them, the chain drops
    them) on chrF, chrT and chrU, written in four sweeps, each in descending
    order of (contig, position). 48 positions hold 2 to 300 reads, dealt over the
    sweeps, so that a position's reads lie some 2 500 lines apart, in other
    tiles, and several of them side by side in one wave; 300 reads of one
    position in one sweep also cross a round's 256 elements."""
    rng = np.random.default_rng(20261022)
    names = [n for n, _ in g["contigs"]]
    lens = {n: len(r) for n, r in g["contigs"]}
    spots = [(names.index(n), p) for n in ("chrF", "chrT", "chrU") for p in range(1, lens[n] + 1)]
    chosen = rng.choice(len(spots), 48, replace=False)
    depths = [2, 3, 63, 64, 65, 255, 256, 257, 300, 300] + rng.integers(2, 120, 38).tolist()
    sweeps = [[] for _ in range(4)]
    for j, (s, d) in enumerate(zip(chosen.tolist(), depths)):
        for k in range(d):
            sweeps[(k * 4 // d + j) % 4 if d < 300 or j % 2 else j % 4].append(spots[s])   # one of the 300s whole in a sweep
    n_deep = sum(depths)
    rest = rng.choice(len(spots), 10007 - n_deep, replace=True)
    for k, s in enumerate(rest.tolist()):
        sweeps[k % 4].append(spots[s])
    lines, k = [], 0
    for sw in sweeps:
        for c, p in sorted(sw, reverse=True):
            lines.append(SC.line(qname=f"d{k}", rname=names[c], pos=p, mapq=0, seq="ACGTACGTACGTACGTACGT"))
            k += 1
    assert len(lines) == 10007 and len(lines) % TILE and len(lines) > 4 * TILE
    return (SC.HEADER + "".join(ln + "\n" for ln in lines)).encode(), [spots[s] for s in chosen.tolist()], depths


def test_file_order_within_a_position_across_waves_rounds_and_tiles(engine, g, names):
    sam, deep, depths = _deep_text(g)
    seen_apart = 0
    for pick, seed in [("first", 0)] + [("seeded", 1000 + 77 * k) for k in range(8)]:
        d = hcgenome.call_genome(sam, g["contigs"], seed=seed, pick=pick)
        a = hcgenome.call_genome(sam, g["contigs"], seed=seed, pick=pick, sorted_buckets=True)
        assert [w["picked"] for w in a["windows"]] == [w["picked"] for w in d["windows"]], (pick, seed)
        assert a["vcf"] == d["vcf"]
        if pick == "first":      # the lowest record of every deep position, and its reads do lie far apart
            recs, of = a["sam"]["records"], a["sam"]["contig_of"]
            picked = {k for w in a["windows"] for k in w["picked"]}
            for (c, p), depth in zip(deep, depths):
                mine = np.flatnonzero((of == c) & (recs["pos"] == p))
                assert len(mine) >= depth and int(mine[0]) in picked and not picked & set(mine[1:].tolist())
                seen_apart += int(mine[-1] - mine[0]) > 2 * TILE
    assert seen_apart >= 24


# ---- 3. four and five passes, positions past 2^31 and 2^32

def test_a_filler_of_2_to_24_bases_in_front_needs_four_passes(got, g):
    filler = ("chrFill", b"ACGT" * (2 ** 22) + b"ACG")
    assert len(filler[1]) == 2 ** 24 + 3
    table = [filler] + list(g["contigs"])
    a = hcgenome.call_genome(g["sam"], table, seed=20261020, want_site_reads=True, sorted_buckets=True)
    d = hcgenome.call_genome(g["sam"], table, seed=20261020, want_site_reads=True)
    assert_same_result(a, d)
    n_fill = -(-len(filler[1]) // 245)
    assert a["contigs"][0] == dict(name="chrFill", first_window=0, n_windows=n_fill, n_records=0)
    assert not any(w["picked"] for w in a["windows"][:n_fill]) and any(w["picked"] for w in a["windows"][n_fill:])
    assert a["vcf"] == got[("seeded", 20261020)]["vcf"]


_CHILD_BIG = """
import ctypes as C, json, sys
sys.path[:0] = {paths!r}
import hcgenome, hcphmm, genome_cases as GC
hcphmm.ensure_built(); hcphmm.init(0)
g = GC.genome()
sam = b"".join(ln + b"\\n" for ln in g["sam"].split(b"\\n")[:-1] if ln[:1] == b"@" or ln.split(b"\\t")[2] != b"chrT")
out = []
for filler in (0, {filler}):
    table = ([("chrFill", b"ACGT")] if filler else []) + list(g["contigs"])
    p = hcgenome.Prepared(sam, table, 1000, 10, seed=5, sorted_buckets=True)
    if filler:
        p.table[0].ref_len = filler       # declared, not backed: no window of it is sent, so it is never read
    h = p.run()
    n_windows = C.c_int32()
    hcgenome.lib().hc_genome_result_vcf(h, None, None, C.byref(n_windows), None)
    n_real = {n_real}
    first = n_windows.value - n_real
    r = hcgenome.results(h, [n.decode("latin-1") for n in p.names], windows=range(first, n_windows.value))
    p.free(h)
    out.append(dict(n_windows=n_windows.value, first=first, contigs=r["contigs"], vcf=r["vcf"].decode("latin-1"),
                    n_records=len(r["sam"]["line_no"]),
                    windows=[[w[k] for k in ("contig", "padded_begin", "padded_end", "ref_len", "picked", "status",
                                             "asm_status", "kmer_size", "n_haps", "reads")] for w in r["windows"]],
                    sites=[[int(s["region"]), int(s["begin"]), int(s["status"])] for s in r["sites"]]))
print("RESULT " + json.dumps(out))
"""


def test_a_filler_of_2_to_32_bases_needs_five_passes_and_no_memory_of_its_size(engine, g):
    """The text is the fixture's without chrT's lines (chrT stays in the table): in
    windows of 1 000 + 2 * 10 bases chrT's planted insertions make a haplotype
    longer than HC_GT_MAX_HAP_LEN, which the chain refuses whatever the buckets."""
    filler = 2 ** 32 + 5
    n_real = sum(-(-len(r) // 1000) for _, r in g["contigs"])
    here = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD_BIG.format(paths=[here, os.path.dirname(hcgenome.__file__)], filler=filler, n_real=n_real)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HC_GENOME_TRACE="1"), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    plain, big = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    traces = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in p.stderr.splitlines() if ln.startswith("[hc_genome]")]
    assert len(traces) == 2
    n_fill = -(-filler // 1000)
    assert (plain["n_windows"], plain["first"], big["n_windows"], big["first"]) == (n_real, 0, n_fill + n_real, n_fill)
    assert big["contigs"][0] == dict(name="chrFill", first_window=0, n_windows=n_fill, n_records=0)
    assert [dict(c, first_window=c["first_window"] - n_fill) for c in big["contigs"][1:]] == plain["contigs"]
    assert sum(1 for w in plain["windows"] if w[4]) >= 15 and plain["vcf"].count("\n") > 4
    assert [[w[0] - 1] + w[1:] for w in big["windows"]] == plain["windows"]
    assert [[s[0] - n_fill] + s[1:] for s in big["sites"]] == plain["sites"] and plain["sites"]
    assert big["vcf"] == plain["vcf"]
    assert [t["sorted"] for t in traces] == ["1", "1"] and int(traces[0]["sort_passes"]) == 2
    assert int(traces[1]["sort_passes"]) == 5
    # the layout's own bound; the dense buckets would ask 24 bytes per base, about 100 GB
    assert int(traces[1]["tile_bytes"]) <= 64 * big["n_records"] + 16 * big["n_windows"] + 2 ** 20
    assert int(traces[0]["tile_bytes"]) <= 64 * plain["n_records"] + 16 * plain["n_windows"] + 2 ** 20


# ---- 4. depth and error parity

def _with_lines(sam, at, lines):
    """The text with `lines` inserted in front of 1-based line `at`."""
    rows = sam.decode().split("\n")
    return "\n".join(rows[:at - 1] + lines + rows[at - 1:]).encode()


def _outcome(sam, contigs, **kw):
    """("ok", the result) or (the error code, its message)."""
    try:
        return "ok", hcgenome.call_genome(sam, contigs, **kw)
    except hcgenome.GenomeError as e:
        return e.code, e.msg


def _same_failure(sam, contigs, begins, **kw):
    d = _outcome(sam, contigs, **kw)
    a = _outcome(sam, contigs, sorted_buckets=True, **kw)
    assert d[0] == hcphmm.EINVAL and a == d, (a, d)
    assert a[1].startswith(begins) or begins in a[1], a[1]
    return a[1]


def test_depth_bound_is_the_dense_paths(got, g, names):
    def sam(n):
        return (SC.HEADER + "".join(SC.line(qname=f"d{k}", rname="chrU", pos=7, mapq=0, seq="A" * 20) + "\n"
                                    for k in range(n))).encode()
    r = hcgenome.call_genome(sam(4096), g["contigs"], pick="first", sorted_buckets=True)
    first = r["contigs"][names.index("chrU")]["first_window"]
    assert [w["picked"] for w in r["windows"]] == [[0] if k == first else [] for k in range(76)]
    assert_same_result(r, hcgenome.call_genome(sam(4096), g["contigs"], pick="first"))
    _same_failure(sam(4097), g["contigs"], "more than 4096 reads begin at position 7 (1-based) of contig chrU")
    # two positions too deep, in different contigs and in the other order in the file: the lowest position is named
    two = (sam(4097) + "".join(SC.line(qname=f"e{k}", rname="chrT", pos=3, mapq=0, seq="A" * 20) + "\n"
                               for k in range(4100)).encode())
    _same_failure(two, g["contigs"], "reads begin at position 3 (1-based) of contig chrT")
    assert hcgenome.call_genome(g["sam"], g["contigs"], sorted_buckets=True)["vcf"] == got[("seeded", 0)]["vcf"]


def test_unplaced_and_defective_reads_fail_as_in_the_dense_path(got, g, names):
    base = got[("seeded", 0)]["vcf"]
    n_alt = len(g["contigs"][names.index("chrT_alt")][1])
    long_unknown = "chrNowhere_" + "z" * 100
    cases = [(dict(rname="chrNone"), "RNAME chrNone is not"), (dict(rname="*"), "RNAME * is not"),
             (dict(rname=long_unknown), "RNAME " + long_unknown[:64] + " is not"),
             (dict(rname="chrT_al"), "RNAME chrT_al is not"), (dict(rname="chrT", pos=0), "POS 0 is 0 or past"),
             (dict(rname="chrT_alt", pos=n_alt + 1), f"POS {n_alt + 1} is 0 or past the {n_alt} bases of contig chrT_alt"),
             (dict(rname="chrT_alt", pos=n_alt + 30), "of contig chrT_alt")]
    for k, (kw, text) in enumerate(cases):       # those of test_unplaced_read_fails_or_is_skipped
        at = 20 + 7 * k
        sam = _with_lines(g["sam"], at, [SC.line(qname="unplaced", seq="A" * 60, **kw)])
        msg = _same_failure(sam, g["contigs"], f"line {at}: unplaced read, ")
        assert text in msg, msg
        assert hcgenome.call_genome(sam, g["contigs"], skip_unplaced=True, sorted_buckets=True)["vcf"] == base, kw
    # a defective read that passes the filters
    sam = _with_lines(g["sam"], 50, [SC.line(qname="bad", rname="chrT", pos=700, cigar="59M", seq="A" * 60)])
    _same_failure(sam, g["contigs"], "line 50: a read that passes the flag filters has the CIGAR's")
    # two offenders in different contigs: the lowest line is named, whatever its kind
    sam = _with_lines(g["sam"], 60, [SC.line(rname="chrNone"), SC.line(rname="chrU", cigar="3M")])
    _same_failure(_with_lines(sam, 30, [SC.line(rname="chr", pos=65)]), g["contigs"], "line 30: unplaced")
    _same_failure(sam, g["contigs"], "line 60: unplaced")
    sam = _with_lines(g["sam"], 60, [SC.line(rname="chrU", cigar="3M"), SC.line(rname="chrNone")])
    _same_failure(sam, g["contigs"], "line 60: a read that passes the flag filters has the CIGAR's")
    # a position too deep beside an unplaced read: the lowest word wins across kinds
    deep = "".join(SC.line(qname=f"d{k}", rname="chrT_alt", pos=1, mapq=0, seq="A" * 20) + "\n" for k in range(4097))
    sam = (SC.HEADER + deep + SC.line(rname="chrNone") + "\n").encode()
    _same_failure(sam, g["contigs"], "more than 4096 reads begin at position 1 (1-based) of contig chrT_alt")
    # the engine is usable afterwards
    assert hcgenome.call_genome(g["sam"], g["contigs"], sorted_buckets=True)["vcf"] == base


# ---- 5. edges

def test_edges(engine, g, names):
    def both(sam, contigs=g["contigs"], **kw):
        a = hcgenome.call_genome(sam, contigs, sorted_buckets=True, want_site_reads=True, **kw)
        assert_same_result(a, hcgenome.call_genome(sam, contigs, want_site_reads=True, **kw))
        return a
    a = both(SC.HEADER.encode())                                            # no record
    assert len(a["windows"]) == 76 and not any(w["picked"] for w in a["windows"]) and a["vcf"].count(b"\n") == 4
    a = both((SC.HEADER + SC.line(rname="chrU", pos=7, mapq=0, seq="A" * 20) + "\n").encode())      # one record
    assert [w["picked"] for w in a["windows"] if w["picked"]] == [[0]]
    sam = (SC.HEADER + "".join(SC.line(rname=n, pos=p) + "\n" for n, p in (("chrNone", 5), ("*", 1), ("chrU", 0), ("chrT2", 2)))
           ).encode()
    a = both(sam, skip_unplaced=True)                                       # every record unplaced
    assert len(a["sam"]["line_no"]) == 4 and not any(w["picked"] for w in a["windows"])
    # the last position of a contig that is not the last is a place, and it is that contig's
    sam = _with_lines(g["sam"], 40, [SC.line(qname="last", rname="chrS65", pos=65, mapq=0, seq="A" * 60)])
    a = both(sam)
    w = a["windows"][a["contigs"][names.index("chrS65")]["first_window"]]
    k = w["picked"][-1]
    assert (int(a["sam"]["records"]["pos"][k]), int(a["sam"]["contig_of"][k]), w["ref_len"]) == (65, names.index("chrS65"), 65)
    # windows of one base, padded by one: a read is picked by up to three windows
    small = [c for c in g["contigs"] if c[0] in ("chrT_alt", "chr", "chrT2", "chrS65")]
    rows = [SC.line(qname=f"s{k}", rname=n, pos=p, mapq=0, seq="ACGTACGT") for k, (n, p) in enumerate(
        [("chrS65", 65), ("chr", 1), ("chrT2", 1), ("chr", 64), ("chrT_alt", 40), ("chr", 1), ("chrS65", 1), ("chrT_alt", 2)])]
    a = both((SC.HEADER + "".join(r + "\n" for r in rows)).encode(), small, region_size=1, padding_size=1, pick="first")
    assert len(a["windows"]) == 40 + 64 + 1 + 65
    assert sum(len(w["picked"]) for w in a["windows"]) == 2 + 2 + 1 + 2 + 2 + 2 + 3     # per position, cut at its contig's ends


# ---- 6. selection by flag and environment

_CHILD_SELECT = """
import ctypes as C, json, sys
sys.path[:0] = {paths!r}
import hccontig, hcgenome, hcphmm, genome_cases as GC
hcphmm.ensure_built(); hcphmm.init(0)
g = GC.genome()
out = []
for flag in {flags!r}:
    try:
        r = hcgenome.call_genome(g["sam"], g["contigs"], seed=3, sorted_buckets=flag)
        out.append(["ok", r["vcf"].decode("latin-1")])
    except hcgenome.GenomeError as e:
        out.append([e.code, e.msg])
name, ref = g["contigs"][4]
p = hccontig.Prepared(g["sam"], name, ref, 245, 85, seed=3, skip_unplaced=True)
h = C.c_void_p()
rc = hccontig.lib().hc_contig_call(p.sam, len(p.sam), p.contig, p.ref, len(p.ref), 245, 85, 3, 0, p.flags | 512, C.byref(h))
out.append([rc, hcphmm.lib().hc_phmm_last_error().decode()])
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("value,flags,want", [(None, [False], ["0"]), ("dense", [False, True], ["0", "1"]),
                                              ("sorted", [False], ["1"]), ("bogus", [False, True], None)])
def test_selection_by_flag_and_environment(got, value, flags, want):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HC_GENOME_TRACE="1")
    env.pop("HC_GENOME_BUCKETS", None)
    if value is not None:
        env["HC_GENOME_BUCKETS"] = value
    code = _CHILD_SELECT.format(paths=[here, os.path.dirname(hcgenome.__file__)], flags=flags)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    traces = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in p.stderr.splitlines() if ln.startswith("[hc_genome]")]
    assert res[-1][0] == hcphmm.EINVAL and "unknown flags" in res[-1][1]       # hc_contig_call keeps its dense buckets
    if want is None:
        assert all(r[0] == hcphmm.EINVAL and "HC_GENOME_BUCKETS" in r[1] for r in res[:-1]), res
        return
    assert [t["sorted"] for t in traces] == want
    assert [int(t["sort_passes"]) > 0 for t in traces] == [w == "1" for w in want]
    assert all(int(t["tile_bytes"]) > 0 for t in traces)
    ref = hcgenome.call_genome(GC.genome()["sam"], GC.genome()["contigs"], seed=3)["vcf"].decode("latin-1")
    assert [r for r in res[:-1]] == [["ok", ref]] * len(flags)


# ---- 7. two sorted runs

def test_two_sorted_runs_give_identical_bytes(got, g):
    a = got[("seeded", 20261020)]
    b = hcgenome.call_genome(g["sam"], g["contigs"], seed=20261020, pick="seeded", want_site_reads=True, sorted_buckets=True)
    assert_same_result(a, b)


# ---- 8. the C++ drop-in

def test_dropin_with_sorted_buckets_writes_the_same_file(engine, g, tmp_path):
    exe = tmp_path / "genome_sorted_dropin"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "genome_sorted_dropin.cpp"),
                    "-L", os.path.dirname(hcphmm.LIB_PATH), "-lhcpairhmm",
                    "-Wl,-rpath," + os.path.dirname(hcphmm.LIB_PATH), "-o", str(exe)], check=True)
    sam, fa = tmp_path / "reads.sam", tmp_path / "ref.fa"
    sam.write_bytes(g["sam"])
    fa.write_text("".join(f">{n}\n" + "".join(r.decode()[i:i + 60] + "\n" for i in range(0, len(r), 60)) for n, r in g["contigs"]))
    env = {k: v for k, v in os.environ.items() if k != "HC_GENOME_BUCKETS"}
    files = {}
    for mode in ("dense", "sorted"):
        out = tmp_path / f"{mode}.vcf"
        p = subprocess.run([str(exe), str(sam), str(fa), str(out), "20261020", mode], env=dict(env, HC_GENOME_TRACE="1"),
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert p.stdout.split() == ["contigs", "12", "windows", "76"]
        assert f"sorted={int(mode == 'sorted')}" in p.stderr.split()
        files[mode] = out.read_bytes()
    assert files["sorted"] == files["dense"] and files["dense"].count(b"\n") > 4 + 5
    assert files["dense"] == hcgenome.call_genome(g["sam"], g["contigs"], seed=20261020)["vcf"]
