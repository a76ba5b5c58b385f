"""Digest of the host planner's dry-run plans (hcx_plan_* / hcx_dump_* hooks, no
GPU): per named case n_seg, the grid flag and the SHA-256 of the pairs, order
and waves arrays. Two builds that print the same text plan alike.

    python tools/plan_digest.py
"""
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"), os.path.join(ROOT, "tests")]
import hcphmm  # noqa: E402
import packing_cases as P  # noqa: E402
import test_planner as T  # noqa: E402
import workloads as W  # noqa: E402

L = P.bind(hcphmm.lib())
L.hcx_plan_regions.restype = T.C.c_double
L.hcx_plan_regions.argtypes = [T.C.c_void_p, T.C.c_int32, T.C.c_int, T.C.c_int]


def show(name, env, plan):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    plan()
    for k, v in old.items():
        os.environ.pop(k) if v is None else os.environ.update({k: v})
    pairs, order, n_seg, waves, grid = T.dump(L)
    sha = " ".join(hashlib.sha256(a.tobytes()).hexdigest()[:16] for a in (pairs, order, waves))
    print(f"{name:28s} n_seg={n_seg} grid={grid} waves={len(waves)} {sha}", flush=True)


def flat(b):
    args, keep = hcphmm._flat_args(b)
    return lambda: L.hcx_plan_pairs(*args, 256, 1, 1)


def regions(rs):
    arr, outs, keep = hcphmm._region_array(rs)
    return lambda: L.hcx_plan_regions(arr, len(rs), 256, 1)


show("S1", {}, flat(W.config("S1")))
for n in (3_000, 20_000, None):
    show(f"S2-{n or '1M-last-part'}", {}, flat(W.config("S2", n)))
show("S4", {}, flat(W.config("S4")))
show("uniform", {}, flat(W.generate(5_000, (250, 250), (101, 101), 0.01, seed=3)))
show("one-bin", {"HC_PHMM_SEG_CAP": "50", "HC_PHMM_SEG_Q": "0"}, flat(P.one_bin()))
ragged = [T.ragged_region(700 + k, nr, nh) for k, (nr, nh) in enumerate([(415, 24), (90, 7), (1, 1), (200, 40)])]
ragged.insert(2, ([], []))
for g in "10":
    show(f"ragged grid_plan={g}", {"HC_PHMM_GRID_PLAN": g}, regions(ragged))
for nh in (8, 32, 128):
    for pol in "10":
        show(f"415x{nh} grid_policy={pol}", {"HC_PHMM_GRID_POLICY": pol}, regions([W.region(415, nh)]))
long_haps = W.generate(300, (100, 6000), (50, 250), 0.01, seed=21)
lane = {"HC_PHMM_KERNEL": "lane"}
for name, env in [("auto", {}), ("diag", {"HC_PHMM_KERNEL": "diag"}), ("seg", {**lane, "HC_PHMM_LANE_SEG": "auto"}),
                  ("segall", {**lane, "HC_PHMM_LANE_SEG": "all"})] + [
                      (f"lane{v}", {**lane, "HC_PHMM_LANE_VARIANT": v, "HC_PHMM_LANE_SEG": "off"}) for v in "012"]:
    show(f"flat-300 {name}", env, flat(long_haps))
