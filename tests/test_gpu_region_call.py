"""GPU: hc_region_call (include/hc_region.h) against the composition of the three
existing calls and against the CPU reference chain, bit for bit; the finish
kernels alone against Oracle.normalize; the runs kernel at its edges; flags,
errors and determinism."""
import re

import numpy as np
import pytest

import hcphmm
import region_chain as RC
import region_workloads as RW

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def hcregion(engine):
    import hcregion as m
    return m


@pytest.fixture(scope="module")
def regs():
    return RW.regions(24, RW.SEED)


@pytest.fixture(scope="module")
def comp(engine, regs):
    return RC.composition(regs)


@pytest.fixture(scope="module")
def full(hcregion, regs):
    return hcregion.call_regions(regs, want_L=True, want_site_reads=True, want_cigars=True)


# ---- 1. equals the composition ------------------------------------------------

def test_equals_the_composition(full, comp, regs):
    assert sum(len(r["reads"]) for r in regs) > sum(int(k.sum()) for k in comp["keep"]) > 0
    assert len(comp["sites"]) > 24
    RC.assert_same(full, comp)


def test_equals_the_composition_in_fp64_mode(hcregion, regs, comp):
    exp = RC.composition(regs, use_double=True)
    got = hcregion.call_regions(regs, want_L=True, want_site_reads=True, want_cigars=True, use_double=True)
    RC.assert_same(got, exp)
    # the mode is the call's: fp64-only likelihoods differ from the default mode's somewhere
    assert any(a.tobytes() != b.tobytes() for a, b in zip(exp["L"], comp["L"]))


def test_cigars_passed_in_give_the_same_records(hcregion, regs, full, comp):
    off = [b for al in comp["alignments"] for b, _ in al]
    cig = [c for al in comp["alignments"] for _, c in al]
    got = hcregion.call_regions(RW.with_alignments(regs, off, cig), want_L=True, want_site_reads=True)
    RC.assert_same(got, dict(full, alignments=None))
    RC.assert_same(got, comp)


# ---- 2. equals the CPU reference chain ------------------------------------------

def test_equals_the_cpu_reference_chain(hcregion, regs, oracle_lib, sw_oracle_lib, gt_oracle_lib):
    six = regs[:6]
    exp = RC.cpu_chain(six, oracle_lib, sw_oracle_lib, gt_oracle_lib)
    got = hcregion.call_regions(six, want_L=True, want_site_reads=True, want_cigars=True)
    RC.assert_same(got, exp)


# ---- 3. the finish kernels alone -------------------------------------------------

READ_LENS = (1, 50, 51, 100, 101, 151)


def _threshold(length):
    return min(2.0, np.ceil(length * 0.02)) * -4.0


def _finish_case(rng, nr, nh):
    lens = np.array([READ_LENS[(r + nh) % len(READ_LENS)] for r in range(nr)], np.int32)
    L = np.zeros((nr, nh))
    for r in range(nr):
        thr, mode = _threshold(int(lens[r])), (r + nr) % 8
        if mode in (1, 2, 3):   # best exactly on, one ulp above, one ulp below the threshold
            best = thr if mode == 1 else np.nextafter(thr, 0.0) if mode == 2 else np.nextafter(thr, -np.inf)
            L[r] = best - rng.uniform(0, 10, nh)
            L[r, int(rng.integers(0, nh))] = best
        elif mode == 4:
            L[r] = -3.25
        elif mode == 5:
            L[r] = -np.inf
        elif mode == 7:
            L[r] = rng.uniform(-80, -50, nh)
        else:
            L[r] = rng.uniform(-30, 0, nh)
            if mode == 6:
                L[r, rng.random(nh) < 0.3] = -np.inf
    return L, lens


def test_finish_kernels_equal_oracle_normalize(hcregion, oracle_lib):
    assert {_threshold(n) for n in READ_LENS} == {-4.0, -8.0}
    rng = np.random.default_rng(5)
    mats, lens = [], []
    for nh in (1, 2, 63, 64, 65, 128):
        for nr in (1, 63, 64, 65, 200):
            L, rl = _finish_case(rng, nr, nh)
            mats.append(L)
            lens.append(rl)
    mats += [np.full((65, 3), -100.0), np.full((65, 3), -0.5), np.zeros((0, 4))]   # all removed, none removed, empty
    lens += [np.full(65, 100, np.int32), np.full(65, 100, np.int32), np.zeros(0, np.int32)]
    got = hcregion.finish(mats, lens)
    removed_on_ulp = kept_on_thr = 0
    for k, (L, rl, (gL, gk, order)) in enumerate(zip(mats, lens, got)):
        if L.shape[0] == 0:
            assert gL.shape[0] == 0 and len(gk) == 0
            continue
        eL, ek = oracle_lib.normalize(L, rl)
        assert np.array_equal(gk, ek), f"case {k} {L.shape}: keep flags differ"
        assert gL.tobytes() == np.ascontiguousarray(eL[ek]).tobytes(), f"case {k} {L.shape}: rows differ"
        kept = np.flatnonzero(ek)
        assert np.array_equal(order[:len(kept)], kept) and np.all(order[len(kept):] == -1), f"case {k}: order"
        best = L.max(axis=1)
        thr = np.array([_threshold(int(n)) for n in rl])
        removed_on_ulp += int((~ek & (best == np.nextafter(thr, -np.inf))).sum())
        kept_on_thr += int((ek & (best == thr)).sum())
    assert removed_on_ulp > 0 and kept_on_thr > 0
    assert not got[-3][1].any() and got[-2][1].all()


# ---- 4. the runs kernel at its edges ----------------------------------------------

def _bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _indel_hap(ref, start, stop, step=12):
    """ref with a one-base deletion and a one-base insertion in turn every `step` bases."""
    out, p, k = bytearray(ref[:start]), start, 0
    while p + step <= stop:
        seg = ref[p:p + step]
        out += seg[:-1] if k % 2 == 0 else seg + (b"A" if seg[-1:] != b"A" else b"C")
        p += step
        k += 1
    return bytes(out + ref[p:])


def _reads_from(rng, r, n, length):
    reads, rb, re_ = [], [], []
    W = len(r["ref"])
    for k in range(n):
        src = RW.hap_bases(r["haps"][k % len(r["haps"])])
        ln = min(length, len(src))
        st = int(rng.integers(0, len(src) - ln + 1))
        reads.append((src[st:st + ln], b"I" * ln, b"I" * ln, b"I" * ln, b"+" * ln))
        rb.append(r["padded_begin"] + min(st, W - 1))
        re_.append(r["padded_begin"] + min(W, st + ln))
    return dict(r, reads=reads, read_begin=np.array(rb, np.int64), read_end=np.array(re_, np.int64))


def _edge_regions():
    rng = np.random.default_rng(9)

    def frame(ref, haps, n_reads, length=100, pad=None):
        W = len(ref)
        pad = W // 5 if pad is None else pad
        r = dict(ref=ref, padded_begin=5000, origin_begin=5000 + pad, origin_end=5000 + W - pad, haps=haps)
        return _reads_from(rng, r, n_reads, length)

    def snp(ref, p):
        return ref[:p] + (b"C" if ref[p:p + 1] != b"C" else b"G") + ref[p + 1:]

    out = {}
    w = _bases(rng, 415)
    out["shortcut"] = frame(w, [w, snp(w, 200), snp(snp(snp(w, 150), 200), 250)], 12)
    out["softclip"] = frame(w, [w, _bases(rng, 40) + snp(w, 210)[:380], snp(w, 100)[35:] + _bases(rng, 40)], 12)
    big = _bases(rng, 1023)
    out["w1023"] = frame(big, [big, _indel_hap(big, 300, 560), _indel_hap(big, 100, 1000), snp(big, 500)], 8, 151)
    w64 = _bases(rng, 64)
    out["w64"] = frame(w64, [w64, snp(w64, 30), w64[:20] + w64[22:], w64[:40] + b"TT" + w64[40:]], 6, 40)
    out["w1"] = frame(b"A", [b"A"], 1, 1, pad=0)
    out["w1_two"] = frame(b"G", [b"G", b"T"], 1, 1, pad=0)
    out["h128"] = frame(w, [w] + [snp(w, 90 + 2 * k) for k in range(127)], 10)
    out["h1"] = frame(w, [snp(w, 207)], 5)
    out["reads0"] = frame(w, [w, snp(w, 199)], 0)
    out["reads1"] = frame(w, [w, snp(w, 199)], 1)
    return out


def test_runs_kernel_edges_equal_the_composition(hcregion, engine):
    edges = _edge_regions()
    regs = list(edges.values())
    exp = RC.composition(regs)
    names = list(edges)
    counts = {n: [len(re.findall(r"\d+[MIDS]", c)) for _, c in exp["alignments"][k]] for k, n in enumerate(names)}
    # what the cases are there for
    assert exp["alignments"][names.index("shortcut")][0] == (0, "415M")
    assert any("S" in c for _, c in exp["alignments"][names.index("softclip")])
    assert 32 < counts["w1023"][1] <= 64 and counts["w1023"][2] > 64, counts["w1023"]
    assert [len(r["ref"]) for r in regs].count(1) == 2 and len(edges["w64"]["ref"]) == 64
    assert len(edges["h128"]["haps"]) == 128 and len(edges["h1"]["haps"]) == 1
    assert len(edges["reads0"]["reads"]) == 0 and len(edges["reads1"]["reads"]) == 1
    got = hcregion.call_regions(regs, want_L=True, want_site_reads=True, want_cigars=True)
    RC.assert_same(got, exp)
    assert len(got["sites"]) > 100   # h128 alone has 127 sites


# ---- 5. flags ---------------------------------------------------------------------

def test_without_site_reads_the_lists_are_null(hcregion, regs, full):
    got = hcregion.call_regions(regs, want_L=True, want_cigars=True)
    assert got["sites"] and all(s["keep_is_null"] and s["n_keep"] == 0 for s in got["sites"])
    assert any(s["n_keep"] > 0 and not s["keep_is_null"] for s in full["sites"])
    RC.assert_same(got, full, lists=False)


def _frozen(x):
    """A result as nested plain values, arrays and floats by their bytes."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, float):
        return np.float64(x).tobytes()
    if isinstance(x, dict):
        return {k: _frozen(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_frozen(v) for v in x]
    return x


def test_default_mode_is_the_mode_of_the_latest_init(engine, hcregion):
    """include/hc_pairhmm.h: the mode of the caller's latest hc_phmm_init holds until
    the next one. The aligner, the genotyper and the assembler initialise the engine
    implicitly and must leave it alone: after init(use_double=True) and one call of
    each, use_double=None is fp64 in hc_region_call and in hc_call_windows."""
    import asm_cases
    import call_cases as CC
    import gt_workloads as GW
    import hcasm
    import hccall
    import hcgt
    import hcsw
    import sw_workloads as SWW
    one = RW.regions(1, seed=941, n_variants=(1, 1), n_reads=(4, 4), artefact=False)
    assert len(one[0]["haps"]) == 2 and len(one[0]["reads"]) == 4
    wins = CC.windows(1)
    engine.init(0, use_double=True)
    try:
        hcsw.align_flat(SWW.regions(1, 2, (60, 80), seed=942))
        hcgt.genotype_sites(*GW.sites(1, 2, reads=(4, 4), haps=(2, 2), seed=943))
        hcasm.assemble([asm_cases.random_region(944, reads=(4, 4))])
        reg = {m: hcregion.call_regions(one, want_L=True, use_double=m) for m in (None, True, False)}
        win = {m: hccall.call_windows(wins, want_L=True, use_double=m) for m in (None, True, False)}
    finally:
        engine.init(0, use_double=False)
    L = {m: [w["L"] for w in win[m]["windows"]] for m in win}
    assert reg[True]["L"][0].size > 0 and L[True][0].size > 0
    assert _frozen(reg[None]["L"]) == _frozen(reg[True]["L"]) and _frozen(reg[None]["sites"]) == _frozen(reg[True]["sites"])
    assert _frozen(reg[True]["L"]) != _frozen(reg[False]["L"])   # or the comparison above could not fail
    assert _frozen(L[None]) == _frozen(L[True]) and _frozen(win[None]["sites"]) == _frozen(win[True]["sites"])
    assert _frozen(L[True]) != _frozen(L[False])


def test_accessors_refuse_what_was_not_asked_for(hcregion, regs):
    p = hcregion.Prepared(regs[:2])
    h = p.run(hcregion.flags_of())
    try:
        assert len(p.keep(h, 0)) == len(regs[0]["reads"])
        for fn in (lambda: p.matrix(h, 0), lambda: p.alignment(h, 0, 0)):
            with pytest.raises(hcregion.RegionError) as e:
                fn()
            assert e.value.code == hcphmm.EINVAL and "did not ask" in str(e.value)
    finally:
        p.free(h)


# ---- 6. errors leave the engines usable ---------------------------------------------

def test_errors_leave_the_engines_usable(hcregion, regs, full, comp):
    import hcgt
    good = regs[0]
    aligned = RW.with_alignments(regs[:1], [b for b, _ in comp["alignments"][0]], [c for _, c in comp["alignments"][0]])[0]
    mixed = dict(good, haps=[aligned["haps"][0]] + [dict(h, cigar=None) for h in aligned["haps"][1:]])
    short = (b"", b"", b"", b"", b"")
    bad = [
        ("with and without a CIGAR", mixed),
        ("null pointer", dict(good, ref=None)),
        ("origin outside the padded window", dict(good, origin_end=good["padded_begin"] + 416)),
        ("", dict(good, reads=[short] + good["reads"][1:])),
    ]
    first = [s for s in full["sites"] if s["region"] == 0]
    for what, region in bad:
        with pytest.raises(hcregion.RegionError) as e:
            hcregion.call_regions([regs[1], region], want_site_reads=True)
        assert e.value.code == hcphmm.EINVAL, what
        msg = str(e.value).split(": ", 1)[1]
        assert msg and what in msg, (what, msg)
        # the next good call, and a plain hcgt.call_regions, are right
        got = hcregion.call_regions([good], want_L=True, want_site_reads=True, want_cigars=True)
        RC.assert_same(got, dict(sites=first, keep=full["keep"][:1], L=full["L"][:1], alignments=full["alignments"][:1]))
    plain = hcgt.call_regions(RC._gt_regions([aligned], comp["L"][:1], comp["keep"][:1]))
    RC.gt_restate.assert_same(plain, first)


# ---- 7. deterministic -----------------------------------------------------------------

def test_two_calls_give_identical_bytes(hcregion, regs, full):
    again = hcregion.call_regions(regs, want_L=True, want_site_reads=True, want_cigars=True)
    RC.assert_same(again, full)
    assert [s["alleles"] for s in again["sites"]] == [s["alleles"] for s in full["sites"]]
