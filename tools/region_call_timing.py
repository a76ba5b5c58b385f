#!/usr/bin/env python3
"""Times hc_region_call against the composition it replaces, on 512 generated
regions of 415 reads x 32 haplotypes (region_workloads.sized):

  region_call_ms   (a) hc_region_call with no WANT_* flag
  composition_ms   (b) hc_sw_align_flat, then hc_phmm_compute_likelihoods_ex per
                   region, then hc_gt_call_regions on the kept reads: the three
                   existing calls, unchanged by the region caller, so this is
                   what the same work cost before it. Only the C calls are
                   timed: the caller's own work between them (parsing nothing,
                   but compacting the kept rows and reads) is left out, which
                   favours (b).

Each is the median and range of --reps calls after a warm-up, wall clock around
the C call(s), with the argument structs built once. Also recorded: (b)'s three
parts, the PairHMM of (b) as one batched hc_phmm_cross_regions pass (for
information: it lacks the filter), and the payload bytes each path moves over
PCIe. Writes one JSON file with the library's build id.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"))

import hcgt   # noqa: E402
import hcphmm   # noqa: E402
import hcregion   # noqa: E402
import hcsw   # noqa: E402
import region_workloads as RW   # noqa: E402


def stats(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=512)
    ap.add_argument("--reads", type=int, default=415)
    ap.add_argument("--haps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_call_timing.json"))
    a = ap.parse_args()
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    regs = RW.sized(a.regions, a.reads, a.haps)

    # (a)
    prep = hcregion.Prepared(regs)
    h = prep.run(hcregion.flags_of(use_double=False))
    new_sites = prep.sites(h)
    new_keep = [prep.keep(h, r) for r in range(prep.n)]
    prep.free(h)
    t_new = timed(lambda: prep.free(prep.run(hcregion.flags_of(use_double=False))), a.reps)

    # (b): structs of the three calls, built once from a first pass
    batch = RW.sw_batch(regs)
    sw_args = hcsw._args(batch, hcsw.SW.NEW_SW_PARAMETERS, hcsw.SOFTCLIP, True)
    n_pairs, stride = len(batch["ref_len"]), 512
    sw_off, sw_buf = np.zeros(n_pairs, np.int32), C.create_string_buffer(n_pairs * stride)
    L = hcphmm.lib()

    def run_sw():
        hcsw._check(L.hc_sw_align_flat(*sw_args, sw_off.ctypes.data_as(hcsw._i32p), sw_buf, stride))

    ph = []
    for r in regs:
        ra, ha, keep_alive = hcphmm._structs(r["reads"], r["haps"])
        out = np.zeros((len(r["reads"]), len(r["haps"])), np.float64)
        keep = np.zeros(len(r["reads"]), np.uint8)
        ph.append((ra, len(r["reads"]), ha, len(r["haps"]), out, keep, C.c_int32(0), keep_alive))

    def run_phmm():
        for ra, nr, ha, nh, out, keep, nk, _ in ph:
            hcphmm._check(L.hc_phmm_compute_likelihoods_ex(ra, nr, ha, nh, out.ctypes.data_as(hcphmm._f64p),
                                                           keep.ctypes.data_as(hcphmm._u8p), C.byref(nk), 0))

    run_sw()
    run_phmm()
    cigars = hcsw._decode(sw_buf, n_pairs, stride)
    aligned = RW.with_alignments(regs, sw_off, cigars)
    gt_regs = []
    for r, (_ra, _nr, _ha, _nh, out, keep, _nk, _ka) in zip(aligned, ph):
        k = keep.astype(bool)
        gt_regs.append(dict(ref=r["ref"], padded_begin=r["padded_begin"], origin_begin=r["origin_begin"],
                            origin_end=r["origin_end"], haps=r["haps"], read_begin=r["read_begin"][k],
                            read_end=r["read_end"][k], L=np.ascontiguousarray(out[k])))
    gprep = hcgt.PreparedRegions(gt_regs)
    gh = gprep.run()
    old_sites = gprep.records(gh)
    gprep.free(gh)

    def run_gt():
        gprep.free(gprep.run())

    def run_old():
        run_sw()
        run_phmm()
        run_gt()

    t_old = timed(run_old, a.reps)
    parts = dict(align_flat_ms=stats(timed(run_sw, a.reps)), compute_likelihoods_ms=stats(timed(run_phmm, a.reps)),
                 gt_call_regions_ms=stats(timed(run_gt, a.reps)))
    cross = hcphmm.RegionsCall([(r["reads"], r["haps"]) for r in regs])
    parts["pairhmm_one_batched_pass_ms"] = stats(timed(cross, a.reps))

    same = len(new_sites) == len(old_sites) and all(
        x["begin"] == y["begin"] and x["alleles"] == y["alleles"] and x["genotype_index"] == y["genotype_index"] and
        x["genotype_quality"] == y["genotype_quality"] and
        x["genotype_likelihoods"].tobytes() == y["genotype_likelihoods"].tobytes() for x, y in zip(new_sites, old_sites))
    same = same and all(np.array_equal(k, p[5].astype(bool)) for k, p in zip(new_keep, ph))

    # Payload bytes over PCIe (descriptors and bases, matrices, results; no allocator padding).
    n = len(regs)
    nh = sum(len(r["haps"]) for r in regs)
    R = sum(len(r["reads"]) for r in regs)
    Rk = sum(int(k.sum()) for k in new_keep)
    ref_b = sum(len(r["ref"]) for r in regs)
    hap_b = sum(len(x) for r in regs for x in r["haps"])
    read_b = 5 * sum(len(x[0]) for r in regs for x in r["reads"])
    Lb = 8 * sum(len(r["reads"]) * len(r["haps"]) for r in regs)
    Lkb = 8 * sum(int(k.sum()) * len(r["haps"]) for k, r in zip(new_keep, regs))
    runs = sum(sum(c in "MIDS" for c in x) for x in cigars)
    site_fixed = sum(104 + 28 * 8 + 8 + 4 * len(regs[s["region"]]["haps"]) for s in old_sites)
    lists = 4 * sum(int(new_keep[s["region"]].sum()) for s in old_sites)   # what the scan reserves per site
    phmm_up, phmm_down = read_b + hap_b, Lb   # the PairHMM pass itself: the same in both
    up = dict(region_call=phmm_up + 56 * n + 20 * nh + 52 * nh + ref_b + hap_b + 20 * R + Lb,
              composition=phmm_up + 40 * nh + 4 * nh + ref_b + hap_b + Lkb + ref_b + hap_b + 16 * runs + 20 * nh +
              56 * n + 16 * Rk)
    down = dict(region_call=phmm_down + 28 + site_fixed + R + 4 * n,
                composition=phmm_down + 72 * nh + site_fixed + lists)
    res = dict(workload=dict(regions=n, reads=a.reads, haps=a.haps, sites=len(old_sites), reads_kept=Rk, reads_total=R),
               reps=a.reps, statistic="median, min and max of reps after one warm-up call, wall clock around the C call(s), ms",
               region_call_ms=stats(t_new), composition_ms=stats(t_old), composition_parts=parts,
               speedup_of_medians=round(statistics.median(t_old) / statistics.median(t_new), 3),
               same_records_and_keep=bool(same), upload_bytes=up, download_bytes=down,
               device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"], git=bid["git"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
