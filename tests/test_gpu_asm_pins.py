"""GPU: the assembler (hcasm.assemble) against the reference's own record of the
seeded cases of tests/asm_pin_cases.py, from tests/golden/asm_golden.npz alone:
attempt codes, k, n_paths, haplotype bytes, order and score bits (tie order and
the kept set at the cut of 128 included), and the reduced graph up to vertex
numbering against the reference's on-path edges. The one case on which the
library does not do what the reference does is the row of
asm_pin_cases.DEVIATIONS.

Then what no other test runs: a workgroup that handles several regions in one
workspace slice, and the grow-only workspace after a larger call."""
import random

import pytest
import torch

import asm_pin_cases as P
import asm_util as U
import hcasm

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _engine(engine):
    """Every test here runs on the engine's device, with a library built from this tree."""


@pytest.fixture(scope="module")
def fixture():
    return P.load_fixture()


def expect(c):
    return P.library_expectation(c["record"])[0]


def test_every_case_alone(fixture):
    results = []
    for c in fixture:
        got, = hcasm.assemble([c["region"]], want_graph=True)
        results.append((c["name"], c["record"], got, U.assert_same))
    P.check_table(results)


def test_every_case_in_one_call_shuffled(fixture):
    cases = list(fixture)
    random.Random(7).shuffle(cases)
    got = hcasm.assemble([c["region"] for c in cases], want_graph=True)
    assert len(got) == len(cases)
    P.check_table([(c["name"], c["record"], g, U.assert_same) for c, g in zip(cases, got)])


def test_a_workgroup_that_handles_several_regions(fixture):
    """2 * CUs + 37 regions in one call: asm_graph_kernel's workgroups take a second region in
    the slice they used for the first. A dozen of the smallest cases in turn, every 50th region one of the
    largest, so that the slice is sized by a large region and small regions follow a large one and the reverse."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    n = 2 * cus + 37
    order = P.slot_order(fixture, n, 2 * cus)   # the engine runs min(n, 2 * CUs) slices
    got = hcasm.assemble([c["region"] for c in order], want_graph=True)
    assert len(got) == n
    for k, (c, g) in enumerate(zip(order, got)):
        U.assert_same(g, expect(c), f"{k}: {c['name']}")


def test_workspace_after_a_larger_call(fixture):
    """Large, tiny, large, then a call whose regions have no reads: each equals its record, the third
    equals the first byte for byte (vertex numbers and edge records included)."""
    by_name = {c["name"]: c for c in fixture}
    large = [by_name[n] for n in ("high_k_105", "slot_sizer", "ties_8", "seg_lengths")]
    tiny = [c for c in fixture if c["family"] == "tiny"][:3]
    bare = [dict(c, region=dict(ref=c["region"]["ref"], reads=[])) for c in (by_name["high_k_75"], tiny[0])]

    def call(cases):
        got = hcasm.assemble([c["region"] for c in cases], want_graph=True)
        assert len(got) == len(cases)
        return got

    first = call(large)
    small = call(tiny)
    third = call(large)
    empty = call(bare)
    for cases, got in ((large, first), (tiny, small), (large, third)):
        for c, g in zip(cases, got):
            U.assert_same(g, expect(c), c["name"])
    assert third == first
    for c, g in zip(bare, empty):   # a window alone is its one haplotype, at k = 25
        ref = c["region"]["ref"]
        assert (g["status"], g["kmer_size"], g["n_paths"], g["haps"]) == (P.OK, 25, 1, [(ref, 0.0)]), c["name"]
        assert len(g["graph"]) == len(ref) - 25
