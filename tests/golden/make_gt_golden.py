"""Generate the genotyper golden fixtures.

    python tests/golden/make_gt_golden.py

Writes tests/golden/gt_golden.npz:
  approx_a, approx_b, approx_out   MathUtils::approximate_log10_sum_log10 from the
                                   REFERENCE's own utils/math_utils.hpp, compiled
                                   in place (oracle/_ref/libref_math.so): random
                                   pairs, every table step near the 8.0 tolerance,
                                   ties, rounding half-steps, -DBL_MAX and -inf
  site fixtures                    gt_workloads.sites() inputs and the REFERENCE's
                                   genotype likelihoods / index / quality, from
                                   genotyper.hpp's own marginal_likelihoods,
                                   calculate_genotype_likelihoods and
                                   get_genotype_quality_and_max_genotype_index
                                   compiled in place (oracle/_ref/libref_chain.so)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"))

import oracle  # noqa: E402
import gt_workloads as G  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gt_golden.npz")


def approx_inputs(rng):
    a = list(rng.uniform(-100, 0, 4000))
    b = list(rng.uniform(-100, 0, 4000))
    base = rng.uniform(-50, 0, 3000)
    d = np.concatenate([np.arange(0, 8.0005, 0.0001)[::7][:1500], 8.0 - np.arange(0, 30) * 1e-4,
                        np.arange(0, 1500) * 1e-4 + 5e-5, rng.uniform(0, 9, 1000)])[:3000]
    a += list(base)
    b += list(base + d)
    big = np.finfo(np.float64).max
    ex = [(-big, -big), (-big, -3.0), (-3.0, -big), (-np.inf, -2.0), (-2.0, -np.inf), (-np.inf, -np.inf),
          (0.0, 0.0), (-0.0, 0.0), (-1.0, -9.0), (-9.0, -1.0), (-1.0, -1.0 - 8.0), (-1.0, -1.0 - 7.99995)]
    a += [x for x, _ in ex]
    b += [y for _, y in ex]
    return np.array(a, np.float64), np.array(b, np.float64)


def main():
    ref = oracle.MathReference()
    rng = np.random.default_rng(60)
    a, b = approx_inputs(rng)
    out = dict(approx_a=a, approx_b=b, approx_out=np.array([ref.approx(x, y) for x, y in zip(a, b)]))
    orc = oracle.ChainReference()
    for name, kw in (("std", {}), ("inf", dict(n_regions=6, seed=62, with_inf=True))):
        mats, sites = G.sites(**kw)
        out[f"{name}_n_mats"] = np.array(len(mats))
        for k, m in enumerate(mats):
            out[f"{name}_mat{k}"] = m
        out[f"{name}_site_m"] = np.array([s["m"] for s in sites], np.int32)
        out[f"{name}_site_A"] = np.array([s["n_alleles"] for s in sites], np.int32)
        out[f"{name}_keep"] = np.concatenate([s["keep"] for s in sites])
        out[f"{name}_keep_n"] = np.array([len(s["keep"]) for s in sites], np.int32)
        out[f"{name}_amap"] = np.concatenate([s["hap_allele"] for s in sites])
        gl, gi, gq = [], [], []
        for s in sites:
            x = orc.site(mats[s["m"]], s["keep"], s["hap_allele"], s["n_alleles"])
            gl.append(x[0])
            gi.append(x[1])
            gq.append(x[2])
        out[f"{name}_gl"] = np.concatenate(gl)
        out[f"{name}_gi"] = np.array(gi, np.int32)
        out[f"{name}_gq"] = np.array(gq, np.int32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(a)} approx pairs, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
