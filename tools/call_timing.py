#!/usr/bin/env python3
"""Times hc_call_windows against the calls it chains, on asm_timing.py's shape
with positions, CIGARs, flags and mapping qualities from the generator of the
window caller's tests (tests/call_cases.py): 512 windows of 415 bases, 415 reads
sampled at 101 bases (a read that would end inside an insertion is a few bases
shorter), 2 % of the reads with a soft-clipped front and 2 % with a
soft-clipped back. Three of the windows are the generator's special ones (no reads, all
filtered, no variant).

  call_windows_ms   (a) hc_call_windows
  prep_reads_ms     (b) hc_prep_reads alone
  asm_then_region_ms (c) on the same prepared input (the views hc_prep_reads
                    gives, cut out on the host beforehand), hc_asm_assemble
                    followed by hc_region_call: the two calls the parent commit
                    has. Their two times are added per repetition.
  overhead_ms       (a) - ((b) + (c)), of the medians

Each figure: median, min and max of --reps calls after a warm-up call, wall
clock around the C call; the structs are built outside the timed region and
every call ends in its own device synchronise. phases: the HC_CALL_TRACE=1 and
HC_PREP_TRACE=1 lines of --trace-reps further calls (the prep trace synchronises
after the upload and after the kernel, so its total is not figure (b)).

Writes one JSON file with the figures, what the windows produced, the device
and the commit.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import call_cases as CC   # noqa: E402
import hcasm   # noqa: E402
import hccall   # noqa: E402
import hcphmm   # noqa: E402
import hcprep   # noqa: E402
import hcregion   # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def stats(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def traced(fn, reps, prefixes):
    """Median of every name=value of the library's trace lines (stderr), per prefix."""
    rows = {p: [] for p in prefixes}
    for env in ("HC_CALL_TRACE", "HC_PREP_TRACE"):
        os.environ[env] = "1"
    try:
        for _ in range(reps):
            with tempfile.TemporaryFile() as tmp:
                sys.stderr.flush()
                saved = os.dup(2)
                os.dup2(tmp.fileno(), 2)
                try:
                    fn()
                finally:
                    os.dup2(saved, 2)
                    os.close(saved)
                tmp.seek(0)
                lines = tmp.read().decode().splitlines()
            for p in prefixes:
                line = [ln for ln in lines if ln.startswith(p)][-1]
                rows[p].append(dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in line.split()[1:]))
    finally:
        for env in ("HC_CALL_TRACE", "HC_PREP_TRACE"):
            del os.environ[env]
    return {p: {k: round(statistics.median(r[k] for r in rs), 3) for k in rs[0]} for p, rs in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--reads", type=int, default=415)
    ap.add_argument("--read-len", type=int, default=101)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--soft-clip", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "call_timing.json"))
    a = ap.parse_args()
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    wins = CC.windows(a.windows, a.seed, a.reads, (a.read_len, a.read_len + 1), a.soft_clip)

    # (a), and what the windows produce (the warm-up call)
    call = hccall.Prepared(wins)
    h = call.run(0)
    res = hccall.results(h, call.n)
    call.free(h)
    t_call = timed(lambda: call.free(call.run(0)), a.reps)

    # (b)
    prep = hcprep.Prepared([CC.prep_window(w) for w in wins])
    prep.free(prep.run())
    t_prep = timed(lambda: prep.free(prep.run()), a.reps)

    # (c): the prepared input as a caller of the parent commit would hold it
    regions, asm_of = [], []
    for k, (w, r) in enumerate(zip(wins, res["windows"])):
        p = r["prep"]
        if not p["kept"]:
            continue
        views = []
        for j in p["kept"]:
            rec, rd = p["records"][j], w["reads"][j]
            lo, hi = rec["offset"], rec["offset"] + rec["length"]
            views.append((rd["bases"][lo:hi], rd["quals"][lo:hi], rec["begin"], rec["end"]))
        asm_of.append(k)
        regions.append(dict(ref=w["ref"], reads=[(b, q) for b, q, _, _ in views], views=views))
    asm = hcasm.Prepared(regions)
    ah = asm.run()
    arecs = hcasm.records(ah, asm.n)
    asm.free(ah)
    rin = []
    for k, g, rec in zip(asm_of, regions, arecs):
        if len(rec["haps"]) <= 1:
            continue
        w = wins[k]
        rin.append(dict(ref=w["ref"], padded_begin=w["padded_begin"], origin_begin=w["origin_begin"],
                        origin_end=w["origin_end"], haps=[x[0] for x in rec["haps"]],
                        reads=[(b, q, b"I" * len(b), b"I" * len(b), b"+" * len(b)) for b, q, _, _ in g["views"]],
                        read_begin=np.array([v[2] for v in g["views"]], np.int64),
                        read_end=np.array([v[3] for v in g["views"]], np.int64)))
    reg = hcregion.Prepared(rin)
    reg.free(reg.run(0))
    t_asm, t_reg = [], []
    for _ in range(a.reps):
        t_asm += timed(lambda: asm.free(asm.run()), 1)
        t_reg += timed(lambda: reg.free(reg.run(0)), 1)
    t_chain = [x + y for x, y in zip(t_asm, t_reg)]

    phases = traced(lambda: call.free(call.run(0)), a.trace_reps, ["[hc_call]", "[hc_prep]"])
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True,
                                text=True, check=True).stdout.strip()
    except Exception:
        commit = bid.get("git")
    status = [r["status"] for r in res["windows"]]
    n_reads = sum(len(w["reads"]) for w in wins)
    out = dict(workload=dict(windows=a.windows, window=CC.WINDOW, reads_per_window=a.reads, read_len=a.read_len,
                             seed=a.seed, soft_clip=a.soft_clip, reads=n_reads, cigar_words=sum(len(hcprep.pack_cigar(r["cigar"]))
                                                                         for w in wins for r in w["reads"]),
                             read_bases=sum(r["seq_len"] for w in wins for r in w["reads"])),
               reps=a.reps, statistic="median, min, max of reps after one warm-up call, wall clock around the C call, ms",
               call_windows_ms=stats(t_call), prep_reads_ms=stats(t_prep), asm_then_region_ms=stats(t_chain),
               asm_assemble_ms=stats(t_asm), region_call_ms=stats(t_reg),
               overhead_ms=round(statistics.median(t_call) - statistics.median(t_prep) - statistics.median(t_chain), 3),
               phases=phases, trace_reps=a.trace_reps,
               results=dict(status_counts=[status.count(s) for s in (0, 1, 2)],
                            kept_reads=sum(r["prep"]["n_kept"] for r in res["windows"]),
                            kept_bases=sum(r["prep"]["kept_bases"] for r in res["windows"]),
                            surviving_reads=sum(len(r["reads"]) for r in res["windows"]),
                            haplotypes=sum(len(r["haps"]) for r in res["windows"]),
                            sites=len(res["sites"]), emitted=sum(s["status"] == 0 for s in res["sites"])),
               device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"]), commit=commit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
