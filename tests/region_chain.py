"""The chain the region caller replaces, two ways (shared by the region tests):

cpu_chain     the reference chain on the CPU: oracle.SWOracle, oracle.Oracle
              pairs + normalize, tests/gt_restate.py
composition   the three existing device calls: hcsw.align_flat, then
              hcphmm.compute_likelihoods per region, then hcgt.call_regions on
              the kept reads

Both return what hcregion.call_regions returns with every want_* flag: sites,
keep, L and alignments, plus (cpu_chain) the number of fp64-rescued pairs."""
import numpy as np

import gt_restate
import region_workloads as RW


def _gt_regions(aligned, mats, keeps):
    out = []
    for r, L, k in zip(aligned, mats, keeps):
        out.append(dict(ref=r["ref"], padded_begin=r["padded_begin"], origin_begin=r["origin_begin"],
                        origin_end=r["origin_end"], haps=r["haps"], read_begin=np.asarray(r["read_begin"])[k],
                        read_end=np.asarray(r["read_end"])[k], L=L))
    return out


def _alignments(regs, off, cig):
    out, k = [], 0
    for r in regs:
        out.append([(int(off[k + j]), cig[k + j]) for j in range(len(r["haps"]))])
        k += len(r["haps"])
    return out


def cpu_chain(regs, orc, sw_orc, gt_orc):
    off, cig = sw_orc.batch(RW.sw_batch(regs), nthreads=4)
    aligned = RW.with_alignments(regs, off, cig)
    mats, keeps, rescued = [], [], 0
    for r in regs:
        nr, nh = len(r["reads"]), len(r["haps"])
        if nr == 0:
            mats.append(np.zeros((0, nh)))
            keeps.append(np.zeros(0, bool))
            continue
        res = orc.pairs(RW.pair_batch(r), nthreads=4)
        rescued += int(res["rescued"].sum())
        L, keep = orc.normalize(res["loglik"].reshape(nr, nh), np.array([len(x[0]) for x in r["reads"]], np.int32))
        mats.append(np.ascontiguousarray(L[keep]))
        keeps.append(keep)
    sites = gt_restate.call_regions(_gt_regions(aligned, mats, keeps), gt_orc)
    return dict(sites=sites, keep=keeps, L=mats, alignments=_alignments(regs, off, cig), rescued=rescued)


def composition(regs, use_double=None):
    import hcgt
    import hcphmm
    import hcsw
    off, cig = hcsw.align_flat(RW.sw_batch(regs))
    aligned = RW.with_alignments(regs, off, cig)
    mats, keeps = [], []
    for r in regs:
        nr, nh = len(r["reads"]), len(r["haps"])
        if nr == 0:
            mats.append(np.zeros((0, nh)))
            keeps.append(np.zeros(0, bool))
            continue
        L, kept = hcphmm.compute_likelihoods([RW.hap_bases(h) for h in r["haps"]], r["reads"], use_double)
        ids = {id(x) for x in kept}
        mats.append(np.ascontiguousarray(L))
        keeps.append(np.array([id(x) in ids for x in r["reads"]], bool))
    sites = hcgt.call_regions(_gt_regions(aligned, mats, keeps))
    return dict(sites=sites, keep=keeps, L=mats, alignments=_alignments(regs, off, cig))


def assert_same(got, exp, lists=True):
    """Every field of every site record, keep bytes, matrices by their bytes,
    alignment begins and CIGAR text."""
    assert len(got["keep"]) == len(exp["keep"])
    for r, (a, b) in enumerate(zip(got["keep"], exp["keep"])):
        assert np.array_equal(a, b), f"region {r}: keep bytes differ"
    if "L" in got:
        for r, (a, b) in enumerate(zip(got["L"], exp["L"])):
            assert a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b, np.float64).tobytes(), \
                f"region {r}: matrices differ"
    if "alignments" in got:
        for r, (a, b) in enumerate(zip(got["alignments"], exp["alignments"])):
            assert a is None or a == b, f"region {r}: alignments differ"
    g = got["sites"]
    if not lists:
        g = [dict(s, keep=e["keep"]) for s, e in zip(g, exp["sites"])]
    gt_restate.assert_same(g, exp["sites"])
