"""GPU: the assembler (include/hc_asm.h, hcasm.assemble) against the sequential
restatement of the reference (tests/asm_restate.py): attempt codes and k, the
reduced graph up to vertex numbering, haplotype bases, order and score bits."""
import random

import numpy as np
import pytest

import asm_restate as AR
import asm_util as U
import hcasm

pytestmark = pytest.mark.gpu

NAMES = "abcdefghijklm"


@pytest.fixture(autouse=True)
def _engine(engine):
    """Every test here runs on the engine's device, with a library built from this tree."""


def test_scenarios_cover_the_table():
    assert "".join(name for name, _, _ in U.scenarios()) == NAMES


@pytest.mark.parametrize("name", list(NAMES))
def test_scenario_alone(name):
    reg, exp = next((r, e) for n, r, e in U.scenarios() if n == name)
    got, = hcasm.assemble([reg], want_graph=True)
    U.assert_same(got, exp, name)


def test_scenarios_in_one_call_shuffled():
    sc = list(U.scenarios())
    random.Random(5).shuffle(sc)
    got = hcasm.assemble([r for _, r, _ in sc], want_graph=True)
    assert len(got) == len(sc)
    for g, (name, _, exp) in zip(got, sc):
        U.assert_same(g, exp, name)
    # without the flag: the same haplotypes, and no graph to ask for
    plain = hcasm.assemble([r for _, r, _ in sc])
    assert [p["haps"] for p in plain] == [g["haps"] for g in got]
    p = hcasm.Prepared([sc[0][1]])
    h = p.run(False)
    try:
        with pytest.raises(hcasm.AsmError) as e:
            hcasm.records(h, 1, want_graph=True)
        assert e.value.code == -1
    finally:
        p.free(h)


@pytest.mark.parametrize("part", range(4))
def test_random_regions(part):
    rs = U.random_set()[16 * part:16 * part + 16]
    got = hcasm.assemble([r for r, _ in rs], want_graph=True)
    for k, (g, (_, exp)) in enumerate(zip(got, rs)):
        U.assert_same(g, exp, f"random region {16 * part + k}")
        assert g["status"] != AR.TOO_COMPLEX


def test_same_call_twice_same_bytes():
    regs = [r for _, r, _ in U.scenarios()] + [r for r, _ in U.random_set()[:3]]
    a = hcasm.assemble(regs, want_graph=True)
    b = hcasm.assemble(regs, want_graph=True)
    assert a == b   # vertex numbers and edge records included


def test_chain_into_region_call():
    """hcasm.assemble -> hcregion.call_regions with cigar == NULL equals the
    same call on the restatement's haplotypes."""
    import hcregion
    import region_workloads as RW
    regs = RW.regions(4, seed=19, n_reads=(40, 100))
    asm_in = [dict(ref=r["ref"], reads=[(x[0], x[1]) for x in r["reads"]]) for r in regs]
    got = hcasm.assemble(asm_in)
    exp = [AR.assemble(a["reads"], a["ref"]) for a in asm_in]
    assert all(e["status"] == AR.OK for e in exp) and any(len(e["haps"]) > 1 for e in exp)

    def call(results):
        out = hcregion.call_regions([dict(r, haps=[h[0] for h in res["haps"]]) for r, res in zip(regs, results)])
        sites = [{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in out["sites"]]
        for s in sites:
            s["genotype_likelihoods"] = np.array(s["genotype_likelihoods"], np.float64).view(np.uint64).tolist()
        return sites, [k.tolist() for k in out["keep"]]

    a, b = call(got), call(exp)
    assert len(a[0]) >= 1
    assert a == b
