"""Share of the swept lane-cells (64 lanes x block width x steps of every seg
wave) at each block width, from the host planner's dry-run plan (no GPU) of a
bench workload: what a width that kept another form of the kernel would weigh.
The 1M-pair S2 is planned in parts and the hooks keep the last part's plan: the
figures are that part's.

    python tools/plan_width_share.py [WORKLOAD [PAIRS]] [--json OUT]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"), os.path.join(ROOT, "tests")]
import hcphmm  # noqa: E402
import packing_cases as P  # noqa: E402
import test_planner as T  # noqa: E402
import workloads as W  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if out:
        args.remove(out)
    wl = args[0] if args else "S2"
    n = int(args[1]) if len(args) > 1 else None
    L = P.bind(hcphmm.lib())
    fa, keep = hcphmm._flat_args(W.config(wl, n))
    L.hcx_plan_pairs(*fa, 256, 1, 1)
    pairs, order, n_seg, waves, grid = T.dump(L)
    swept = 64 * waves[:, 3].astype(np.int64) * waves[:, 5]
    rows = []
    for bc in sorted(set(waves[:, 3].tolist())):
        m = waves[:, 3] == bc
        rows.append(dict(workload=wl, pairs_planned=int(n_seg), width=int(bc), waves=int(m.sum()),
                         share_of_swept_lane_cells=round(float(swept[m].sum() / swept.sum()), 4)))
    for r in rows:
        print(json.dumps(r))
    if out:
        with open(out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
