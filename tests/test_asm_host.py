"""CPU: the host half of the assembler (include/hc_asm.h). The path enumeration,
scores, order and bytes through the hcx_asm_paths_from_graph hook against the
restatement, the HC_PHMM_EINVAL cases (raised before any device work), the
TOO_COMPLEX cap, and the stand-alone host program under the host sanitizers:
asm_paths.cpp on its own, and the text of the device's graph phases compiled
for one host thread."""
import ctypes as C
import subprocess

import pytest

import asm_restate as AR
import asm_util as U
import hcasm
import hcphmm

EINVAL = -1


def test_exports_and_mirror():
    syms = hcasm.declared_symbols()
    assert syms == ["hc_asm_assemble", "hc_asm_result_free", "hc_asm_result_graph", "hc_asm_result_hap",
                    "hc_asm_result_region"]
    out = subprocess.run(["nm", "-D", "--defined-only", hcphmm.LIB_PATH], check=True, capture_output=True, text=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines()}
    assert set(syms) <= exported and "hcx_asm_paths_from_graph" in exported
    assert hcasm.mirrored_symbols() == syms


def _hook(res):
    g = res["g"]
    return hcasm.paths_from_graph(g.ref[:res["kmer_size"]], res["graph"], res["source"], res["sink"])


@pytest.mark.parametrize("name", [n for n, _, _ in U.scenarios() if n != "h"])
def test_hook_equals_restatement_on_scenarios(name):
    exp = next(e for n, _, e in U.scenarios() if n == name)
    got = _hook(exp)
    assert got["status"] == AR.OK and got["n_paths"] == exp["n_paths"]
    assert [h[0] for h in got["haps"]] == [h[0] for h in exp["haps"]]
    assert [U.score_bits(h[1]) for h in got["haps"]] == [U.score_bits(h[1]) for h in exp["haps"]]
    assert got["graph"] == exp["graph"] and (got["source"], got["sink"]) == (exp["source"], exp["sink"])


def test_hook_equals_restatement_on_random_regions():
    n_multi = 0
    for k, (_, exp) in enumerate(U.random_set()):
        if exp["status"] != AR.OK:
            continue
        got = _hook(exp)
        assert [(h[0], U.score_bits(h[1])) for h in got["haps"]] == \
            [(h[0], U.score_bits(h[1])) for h in exp["haps"]], k
        n_multi += len(exp["haps"]) > 2
    assert n_multi >= 16


def test_hook_does_not_need_a_reduced_graph():
    """Edges no path uses (a dangling tail, a side entry) take no part in the scores."""
    exp = next(e for n, _, e in U.scenarios() if n == "b")
    nv = len(exp["g"].kmer)
    extra = exp["graph"] + [(exp["graph"][3][0], nv, ord("A"), 7, 0, 9000), (nv + 1, exp["graph"][5][1], ord("C"), 9, 0, 9001)]
    got = hcasm.paths_from_graph(exp["g"].ref[:25], extra, exp["source"], exp["sink"])
    assert [(h[0], U.score_bits(h[1])) for h in got["haps"]] == [(h[0], U.score_bits(h[1])) for h in exp["haps"]]


def _bubbles(n):
    edges = []
    for b in range(n):
        for br in range(2):
            mid = 3 * b + 1 + br
            edges.append((3 * b, mid, b"AC"[br], 2 + br, 0, len(edges)))
            edges.append((mid, 3 * b + 3, ord("G"), 2 + br, 0, len(edges)))
    return edges


def test_too_complex_is_a_status():
    over = hcasm.paths_from_graph(b"T" * 25, _bubbles(17), 0, 51)   # 131 072 paths
    assert (over["status"], over["n_paths"], over["haps"]) == (hcasm.TOO_COMPLEX, hcasm.MAX_PATHS + 1, [])
    at = hcasm.paths_from_graph(b"T" * 25, _bubbles(16), 0, 48)     # exactly the cap
    assert (at["status"], at["n_paths"], len(at["haps"])) == (hcasm.OK, hcasm.MAX_PATHS, hcasm.MAX_HAPS)
    # stable order among the equal scores of the best paths: discovery order
    best = at["haps"][0][1]
    assert best == max(h[1] for h in at["haps"])
    assert at["haps"][0][0] == b"T" * 25 + b"CG" * 16


def test_tie_rule_is_discovery_order():
    """Two branches of equal count: equal scores, the first out-edge first."""
    edges = [(0, 1, ord("A"), 3, 1, 0), (0, 2, ord("C"), 3, 0, 1), (1, 3, ord("G"), 3, 1, 2), (2, 3, ord("G"), 3, 0, 3)]
    got = hcasm.paths_from_graph(b"ACGTA", edges, 0, 3)
    assert [h[0] for h in got["haps"]] == [b"ACGTAAG", b"ACGTACG"]
    assert got["haps"][0][1] == got["haps"][1][1]


def test_source_equal_sink_is_one_haplotype():
    got = hcasm.paths_from_graph(b"ACGTACGTACGTACGTACGTACGTA", [], 4, 4)
    assert (got["status"], got["n_paths"], got["haps"]) == (hcasm.OK, 1, [(b"ACGTACGTACGTACGTACGTACGTA", 0.0)])


def _rc(regions, n=None, flags=0, out=True):
    L = hcasm.lib()
    p = hcasm.Prepared(regions) if not isinstance(regions, (type(None), C.Array)) else None
    arr = p.arr if p else regions
    h = C.c_void_p()
    rc = L.hc_asm_assemble(arr, len(regions) if n is None else n, flags, C.byref(h) if out else None)
    msg = L.hc_phmm_last_error()
    assert not h.value or rc == 0
    if h.value:
        L.hc_asm_result_free(h)
    return rc, (msg or b"").decode()


def test_einval_before_any_device_work():
    ok = dict(ref=b"A" * 50, reads=[(b"ACGT", b"IIII")])
    assert _rc([ok], out=False)[0] == EINVAL
    assert _rc(None, n=1)[0] == EINVAL
    assert _rc([ok], n=-1)[0] == EINVAL
    assert _rc([ok], flags=2)[0] == EINVAL
    rc, msg = _rc([ok, dict(ref=None, reads=[])])
    assert rc == EINVAL and "region 1" in msg
    assert _rc([dict(ref=b"", reads=[])])[0] == EINVAL                       # ref_len 0
    assert _rc([dict(ref=b"A" * 1024, reads=[])])[0] == EINVAL              # > HC_GT_MAX_REF_LEN
    rc, msg = _rc([dict(ref=b"A" * 50, reads=[(b"ACGT", None)])])
    assert rc == EINVAL and "quals" in msg
    rc, msg = _rc([dict(ref=b"A" * 50, reads=[(b"A" * 65537, b"I" * 65537)])])
    assert rc == EINVAL and "longer" in msg
    rc, msg = _rc([dict(ref=b"A" * 50, reads=[(b"A" * 65536, b"I" * 65536)] * 3)])
    assert rc == EINVAL and "read bases" in msg
    # struct-level cases
    arr = (hcasm.Region * 1)()
    arr[0] = hcasm.Region(b"A" * 50, 50, None, -1)
    assert _rc(arr, n=1)[0] == EINVAL
    arr[0] = hcasm.Region(b"A" * 50, 50, None, 2)
    assert _rc(arr, n=1)[0] == EINVAL
    ra = (hcasm.Read * 1)()
    ra[0] = hcasm.Read(b"ACGT", b"IIII", -4)
    arr[0] = hcasm.Region(b"A" * 50, 50, ra, 1)
    assert _rc(arr, n=1)[0] == EINVAL
    ra[0] = hcasm.Read(None, b"IIII", 4)
    assert _rc(arr, n=1)[0] == EINVAL


def test_empty_call_and_accessor_errors():
    L = hcasm.lib()
    h = C.c_void_p()
    assert L.hc_asm_assemble(None, 0, 0, C.byref(h)) == 0 and h.value
    assert L.hc_asm_result_region(h, 0, None, None, None, None, None) == EINVAL
    assert L.hc_asm_result_hap(h, 0, 0, None, None, None) == EINVAL
    assert L.hc_asm_result_free(h) == 0
    assert L.hc_asm_result_region(None, 0, None, None, None, None, None) == EINVAL
    assert L.hc_asm_result_free(None) == 0


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/asm_host_main.cpp with -fsanitize=address,undefined: asm_paths.cpp
    on (b), (i) and the 17-bubble graph; and the device's graph phases as one host
    thread runs them, on every scenario, equal to the restatement."""
    exe = U.build_host_main(tmp_path)
    sc = {n: (r, e) for n, r, e in U.scenarios()}
    for name in "bi":
        exp = sc[name][1]
        fin, fout = tmp_path / f"g_{name}.txt", tmp_path / f"g_{name}.out"
        fin.write_text(U.graph_input(exp["kmer_size"], exp["g"].ref[:exp["kmer_size"]], exp["graph"], exp["source"],
                                     exp["sink"]))
        subprocess.run([exe, "graph", str(fin), str(fout)], check=True, timeout=120)
        got, = U.parse_out(fout.read_text())
        assert [(h[0], U.score_bits(h[1])) for h in got["haps"]] == [(h[0], U.score_bits(h[1])) for h in exp["haps"]]
        assert got["n_paths"] == exp["n_paths"]
    out = subprocess.run([exe, "bubbles", "17"], check=True, capture_output=True, text=True, timeout=120).stdout
    got, = U.parse_out(out)
    assert (got["status"], got["n_paths"], got["haps"]) == (hcasm.TOO_COMPLEX, hcasm.MAX_PATHS + 1, [])
    fin, fout = tmp_path / "emul.txt", tmp_path / "emul.out"
    fin.write_text(U.emul_input([r for r, _ in sc.values()]))
    subprocess.run([exe, "emul", str(fin), str(fout)], check=True, timeout=120)
    got = U.parse_out(fout.read_text())
    assert len(got) == len(sc)
    for g, (name, (_, exp)) in zip(got, sc.items()):
        U.assert_same(g, exp, name)
