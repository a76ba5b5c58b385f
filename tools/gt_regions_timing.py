#!/usr/bin/env python3
"""Times hc_gt_call_regions on the bench's genotyper workload shape (512 regions
x 16 sites, 415 reads x 32 haplotypes) against what it replaces:

  call_regions_ms     hc_gt_call_regions, regions in, site records out
  genotype_sites_ms   hc_gt_genotype_sites on the same sites with the maps and
                      keep lists precomputed outside the timed region
  host_bookkeeping_ms the bookkeeping a caller of hc_gt_genotype_sites does
                      itself, restated in C++ (tests/cpp/gt_dropin.cpp, `host`
                      mode), one core

Each is the median of --reps calls after a warm-up. Writes one JSON file with
the three figures, the bytes each path moves, the device and the commit.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"))

import gt_workloads as G   # noqa: E402
import hcgt   # noqa: E402
import hcphmm   # noqa: E402


def build(n_regions, sites_per_region, n_reads, n_haps, seed=63, window=415, origin=245):
    """Regions with exactly sites_per_region sites: edits on a grid inside the
    origin, far enough apart not to interact, each carried by some haplotype."""
    rng = np.random.default_rng(seed)
    out = []
    first = (window - origin) // 2 + 4
    step = (origin - 8) // sites_per_region
    assert step >= 8
    for _ in range(n_regions):
        ref = G.ACGT[rng.integers(0, 4, window)].tobytes()
        pool = []
        for k in range(sites_per_region):
            pos, t = first + k * step, rng.random()
            if t < 0.7:
                pool.append((pos, 0, "S", int([b for b in G.ACGT if b != ref[pos]][int(rng.integers(0, 3))])))
            elif t < 0.85:
                pool.append((pos, 1, "I", G.ACGT[rng.integers(0, 4, int(rng.integers(1, 5)))].tobytes()))
            else:
                pool.append((pos, 2, "D", int(rng.integers(1, 5))))
        haps = [dict(bases=ref, begin=0, cigar=f"{window}M")]
        for h in range(1, n_haps):
            pick = [e for k, e in enumerate(pool) if rng.random() < 0.3 or 1 + k % (n_haps - 1) == h]
            bases, cigar, _ = G.apply_edits(ref, pick)
            haps.append(dict(bases=bases, begin=0, cigar=cigar))
        pb = int(rng.integers(1000, 1_000_000))
        rb = pb + rng.integers(-60, window - 40, n_reads)
        out.append(dict(ref=ref, padded_begin=pb, origin_begin=pb + (window - origin) // 2,
                        origin_end=pb + (window - origin) // 2 + origin, haps=haps,
                        read_begin=rb.astype(np.int64), read_end=(rb + rng.integers(70, 151, n_reads)).astype(np.int64),
                        L=G.region_matrix(rng, n_reads, n_haps)))
    return out


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=512)
    ap.add_argument("--sites", type=int, default=16)
    ap.add_argument("--reads", type=int, default=415)
    ap.add_argument("--haps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_regions_timing.json"))
    a = ap.parse_args()
    import torch
    bid = hcphmm.ensure_built()
    regs = build(a.regions, a.sites, a.reads, a.haps)
    prep = hcgt.PreparedRegions(regs)
    recs = prep.records(prep.run())
    assert len(recs) == a.regions * a.sites, len(recs)
    new = median_ms(lambda: prep.free(prep.run()), a.reps)
    live = [r for r in recs if r["status"] != hcgt.TOO_MANY_ALLELES]
    sites = [dict(m=r["region"], keep=r["keep"], hap_allele=r["hap_allele"], n_alleles=r["n_alleles"]) for r in live]
    base = hcgt.Prepared([r["L"] for r in regs], sites)
    old = median_ms(base.run, a.reps)
    same = all(np.array_equal(g[0].view(np.uint64), r["genotype_likelihoods"].view(np.uint64)) and
               g[1:] == (r["genotype_index"], r["genotype_quality"]) for g, r in zip(base.results(), live))
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin = os.path.join(tmp, "gt_dropin"), os.path.join(tmp, "in.bin")
        libdir = os.path.dirname(hcphmm.LIB_PATH)
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "gt_dropin.cpp"), "-L", libdir, "-lhcpairhmm",
                        "-Wl,-rpath," + libdir, "-o", exe], check=True)
        G.write_regions(fin, regs)
        host = subprocess.run(["taskset", "-c", "0", exe, "host", fin, "5"], check=True, capture_output=True,
                              text=True).stdout.split()
    sums = [len(recs), sum(len(r["keep"]) for r in recs), sum(int(r["hap_allele"].sum()) for r in recs),
            sum(len(x) for r in recs for x in r["alleles"])]
    L_bytes = sum(r["L"].nbytes for r in regs)
    runs = sum(sum(c in "MIDS" for c in h["cigar"]) for r in regs for h in r["haps"])
    n_haps = sum(len(r["haps"]) for r in regs)
    up_new = (L_bytes + sum(len(r["ref"]) + sum(len(h["bases"]) for h in r["haps"]) + 16 * len(r["read_begin"])
                            for r in regs) + 16 * runs + 20 * n_haps + 56 * len(regs))
    up_old = L_bytes + 4 * sum(len(s["keep"]) + len(s["hap_allele"]) for s in sites) + 40 * len(sites)
    down_new = sum(104 + 28 * 8 + 8 + 4 * (len(regs[r["region"]]["read_begin"]) + len(regs[r["region"]]["haps"]))
                   for r in recs)
    down_old = sum(8 * len(g[0]) + 8 for g in base.results())
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True,
                                text=True, check=True).stdout.strip()
    except Exception:
        commit = bid.get("git")
    res = dict(workload=dict(regions=a.regions, sites_per_region=a.sites, reads=a.reads, haps=a.haps, sites=len(recs)),
               reps=a.reps, statistic="median of reps after one warm-up call, wall clock around the C call, ms",
               call_regions_ms=round(new[0], 3), call_regions_min_max_ms=[round(new[1], 3), round(new[2], 3)],
               genotype_sites_ms=round(old[0], 3), genotype_sites_min_max_ms=[round(old[1], 3), round(old[2], 3)],
               host_bookkeeping_ms=round(float(host[0]), 3), host_bookkeeping_cores=1,
               host_bookkeeping_matches_device=[int(x) for x in host[1:]] == sums,
               same_arithmetic_bits=bool(same),
               upload_bytes=dict(call_regions=up_new, genotype_sites=up_old),
               download_bytes=dict(call_regions=down_new, genotype_sites=down_old),
               device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"]),
               commit=commit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
