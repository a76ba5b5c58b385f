"""CPU: the assembler pinned to the reference compiled in place.

tests/golden/asm_golden.npz holds, for the seeded cases of tests/asm_pin_cases.py,
what the reference's own assembler/assembler.hpp and assembler/graph_wrapper.hpp
did (oracle/ref_asm_driver.cpp over a stand-in for Boost.Graph). Against it:

  * the restatement (tests/asm_restate.py), exact except inside runs of equal
    score bits, where its stable sort and the reference's std::sort may order,
    and at the cut of 128 choose, differently;
  * the library's host half (hcasm.paths_from_graph) on the reference's graphs,
    exact, tie order and the kept set at the cut included;
  * the device's graph phases compiled for one host thread, and asm_paths.cpp,
    in tests/cpp/asm_host_main.cpp under the host sanitizers, exact;
  * asm_pin_cases.DEVIATIONS, the one row on which the library does not do what
    the reference does.

Where oracle/_ref/libref_asm.so is built, the same live: the fixture is what
the reference gives now, and seeded random regions through both.
"""
import os
import random
import subprocess

import pytest

import asm_cases as AC
import asm_pin_cases as P
import asm_restate as AR
import asm_util as U
import hcasm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return P.load_fixture()


@pytest.fixture(scope="module")
def reference():
    import oracle
    if not oracle.asm_reference_available():
        pytest.skip("oracle/_ref/libref_asm.so is not built (the reference tree is absent): "
                    "the committed fixture is the pin")
    return oracle.AsmReference()


@pytest.fixture(scope="module")
def host_main(tmp_path_factory):
    return U.build_host_main(tmp_path_factory.mktemp("asm_host_main"))


# ---- the restatement ------------------------------------------------------------------------

def check_restatement(reg, rec, what):
    res = AR.assemble(reg["reads"], reg["ref"])
    assert res["attempts"] == rec["attempts"], (what, res["attempts"], rec["attempts"])
    assert res["kmer_size"] == rec["kmer_size"], what
    if rec["n_paths"] > AR.MAX_PATHS:
        assert (res["status"], res["n_paths"], res["haps"]) == (AR.TOO_COMPLEX, AR.MAX_PATHS + 1, []), what
        return res
    assert (res["status"], res["n_paths"]) == (rec["status"], rec["n_paths"]), what
    all_sorted = res["g"].sorted_haps if res["g"] is not None and res["status"] == AR.OK else []
    P.assert_equal_up_to_ties(res["haps"], all_sorted, rec["haps"], rec["n_paths"], what)
    if rec["status"] == P.OK:
        assert U.canon_graph(res["graph"], res["source"], res["sink"]) == \
            U.canon_graph(P.on_path_graph(rec), rec["source"], rec["sink"]), what
    return res


def test_restatement_equals_the_reference_on_the_fixture(fixture):
    differs = []
    for c in fixture:
        res = check_restatement(c["region"], c["record"], c["name"])
        if not P.same_as_reference(res, c["record"]):
            differs.append(c["name"])
    # the finding: std::sort is not the stable sort once more than 16 paths tie
    assert "ties_3" not in differs and "ties_4" not in differs
    assert {"ties_5", "ties_8", "bubbles_17"} <= set(differs), differs
    assert all(n.startswith("ties_") or n == "bubbles_17" for n in differs), differs


def test_the_reference_keeps_another_set_than_the_stable_sort_at_the_cut(fixture):
    for name in ("ties_8", "ties_8_skew"):
        c = next(c for c in fixture if c["name"] == name)
        res = AR.assemble(c["region"]["reads"], c["region"]["ref"])
        kept = c["record"]["haps"]
        assert sorted(h[0] for h in res["haps"]) != sorted(h[0] for h in kept), name
        # the run of equal score bits at the cut goes on behind it
        last = U.score_bits(kept[-1][1])
        in_all = sum(U.score_bits(h[1]) == last for h in res["g"].sorted_haps)
        assert in_all > len(P.runs(kept)[-1][1]) >= 2, name
        if name == "ties_8_skew":   # and the run in front of it scores differently: unequal neighbours
            assert len(P.runs(kept)) >= 10 and U.score_bits(kept[-1 - len(P.runs(kept)[-1][1])][1]) != last
    c = next(c for c in fixture if c["name"] == "ties_5")
    res = AR.assemble(c["region"]["reads"], c["region"]["ref"])
    assert sorted(h[0] for h in res["haps"]) == sorted(h[0] for h in c["record"]["haps"])
    assert [h[0] for h in res["haps"]] != [h[0] for h in c["record"]["haps"]]


def test_restatement_equals_the_reference_live(reference):
    seeds = list(range(7100, 7124))
    n_multi = 0
    for seed in seeds:
        reg = AC.random_region(seed)
        rec = reference.assemble(reg["reads"], reg["ref"])
        check_restatement(reg, rec, f"random region {seed}")
        n_multi += len(rec["haps"]) > 1
    assert n_multi >= 8
    for n in (2, 5, 7):
        reg = P.snp_ladder(7200 + n, n)
        check_restatement(reg, reference.assemble(reg["reads"], reg["ref"]), f"ladder {n}")


def test_fixture_is_what_the_reference_gives_now(reference, fixture):
    assert [(c["family"], c["name"]) for c in fixture] == [(f, n) for f, n, _ in P.all_cases()]
    for c, (_, _, reg) in zip(fixture, P.all_cases()):
        assert c["region"] == reg, c["name"]
        now = reference.assemble(reg["reads"], reg["ref"])
        assert P.encode([(c["family"], c["name"], reg, now)]) == P.encode([(c["family"], c["name"], reg, c["record"])]), c["name"]


def test_census_of_the_families(fixture):
    """Read off the reference's records, so a regenerated fixture cannot lose a family's edge quietly."""
    P.census({c["name"]: c["record"] for c in fixture})
    assert {c["family"] for c in fixture} == set(P.FAMILIES)
    assert os.path.getsize(P.GOLDEN) < (1 << 20)


# ---- the stand-in -----------------------------------------------------------------------------

def test_graph_standin_program(tmp_path):
    """The container and the DFS under the reference's assembler, on their own, under the host sanitizers."""
    exe = tmp_path / "graph_standin_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "oracle", "boost_standin"),
                    os.path.join(ROOT, "tests", "cpp", "graph_standin_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120)
    assert out.stdout.strip() == "ok"


# ---- the library's host half --------------------------------------------------------------------

def compare_haps(got, exp, what):
    assert (got["status"], got["n_paths"]) == (exp["status"], exp["n_paths"]), what
    assert [h[0] for h in got["haps"]] == [h[0] for h in exp["haps"]], what
    assert [U.score_bits(h[1]) for h in got["haps"]] == [U.score_bits(h[1]) for h in exp["haps"]], what


def with_graph(fixture):
    return [c for c in fixture if c["record"]["kmer_size"]]


def test_hook_equals_the_reference_on_the_fixture_graphs(fixture):
    """hcasm.paths_from_graph on the reference's on-path edges: haplotype bytes, order and score bits."""
    results = []
    for c in with_graph(fixture):
        rec = c["record"]
        got = hcasm.paths_from_graph(c["region"]["ref"][:rec["kmer_size"]], P.on_path_graph(rec), rec["source"], rec["sink"])
        results.append((c["name"], rec, dict(got, attempts=rec["attempts"], kmer_size=rec["kmer_size"]), compare_haps))
    assert len(results) >= 80
    P.check_table(results)


def test_hook_on_the_whole_graphs_too(fixture):
    """Edges no path uses, the filtered ones among them, may be handed in: only for graphs whose every
    edge passes the filter is that the same walk, so those are the ones compared."""
    n = 0
    for c in with_graph(fixture):
        rec = c["record"]
        if rec["n_paths"] > P.MAX_PATHS or not all(e[3] >= 2 or e[4] for e in rec["edges"]):
            continue
        whole = [(u, v, base, count, is_ref, seq) for u, v, base, count, is_ref, _, seq in rec["edges"]]
        got = hcasm.paths_from_graph(c["region"]["ref"][:rec["kmer_size"]], whole, rec["source"], rec["sink"])
        compare_haps(got, rec, c["name"])
        n += 1
    assert n >= 20


# ---- the host program under the sanitizers --------------------------------------------------------

def test_host_program_graph_mode_on_the_fixture(fixture, host_main, tmp_path):
    results = []
    for c in with_graph(fixture):
        rec = c["record"]
        fin, fout = tmp_path / "g.txt", tmp_path / "g.out"
        fin.write_text(U.graph_input(rec["kmer_size"], c["region"]["ref"][:rec["kmer_size"]], P.on_path_graph(rec),
                                     rec["source"], rec["sink"]))
        subprocess.run([host_main, "graph", str(fin), str(fout)], check=True, timeout=120)
        got, = U.parse_out(fout.read_text())
        results.append((c["name"], rec, dict(got, attempts=rec["attempts"], kmer_size=rec["kmer_size"]), compare_haps))
    P.check_table(results)


def run_emul(host_main, tmp_path, mode, regions):
    fin, fout = tmp_path / f"{mode}.txt", tmp_path / f"{mode}.out"
    fin.write_text(U.emul_input(regions))
    subprocess.run([host_main, mode, str(fin), str(fout)], check=True, timeout=300)
    got = U.parse_out(fout.read_text())
    assert len(got) == len(regions)
    return got


def test_host_program_emul_mode_on_the_fixture(fixture, host_main, tmp_path):
    """The device's graph phases as one host thread runs them, the segment arithmetic lane by lane."""
    got = run_emul(host_main, tmp_path, "emul", [c["region"] for c in fixture])
    P.check_table([(c["name"], c["record"], g, U.assert_same) for c, g in zip(fixture, got)])


def test_host_program_one_slot_for_many_regions(fixture, host_main, tmp_path):
    """asm_graph_kernel's loop over the regions of one slice: small after large and large after small,
    nothing cleared in between but what every attempt resets itself."""
    order = P.slot_order(fixture, 120, 40)
    got = run_emul(host_main, tmp_path, "emulslot", [c["region"] for c in order])
    for k, (c, g) in enumerate(zip(order, got)):
        U.assert_same(g, P.library_expectation(c["record"])[0], f"{k}: {c['name']}")


def test_shuffled_one_slot(fixture, host_main, tmp_path):
    cases = [c for c in fixture if c["family"] in ("seg", "degenerate", "filter", "refused", "limit", "slot")]
    random.Random(11).shuffle(cases)
    got = run_emul(host_main, tmp_path, "emulslot", [c["region"] for c in cases])
    for c, g in zip(cases, got):
        U.assert_same(g, P.library_expectation(c["record"])[0], c["name"])
