#!/usr/bin/env python3
"""Times hc_asm_assemble on generated regions of the region caller's timing
shape: 512 regions, 415-base windows, 415 reads x 101 bases, 0-3 variants on a
second haplotype, 0.1 % read errors (--err; at 0.5 % the error k-mers of 415
reads alone pass the 2000 unique k-mers and every region climbs to k = 95).

  assemble_ms   median, min and max of --reps calls after a warm-up, wall clock
                around the C call (structs built outside the timed region)
  phases_ms     the same call with HC_ASM_TRACE=1 (which synchronises after the
                upload and after the kernels, so its total is not the figure
                above): layout, upload, device graph, readback, host paths;
                median of --trace-reps calls. walk_share is the part of the
                regions' device time (their own clock, summed) that the
                single-thread threading takes; slowest_region_ms and
                its_walk_ms are the slowest region's time and threading

Writes one JSON file with the figures, what the regions produced, the device
and the commit. There is no baseline to compare with: the parent commit has no
assembler and the reference's does not build without Boost.Graph.
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

import hcasm   # noqa: E402
import hcphmm   # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def build(n_regions, window, n_reads, read_len, seed=77, err=0.001):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_regions):
        ref = ACGT[rng.integers(0, 4, window)]
        alt = ref.copy()
        nvar = int(rng.integers(0, 4))
        for pos in sorted(rng.integers(40, window - 40, nvar).tolist(), reverse=True):
            kind = int(rng.integers(0, 3))
            if kind == 0:
                alt[pos] = ACGT[(int(np.flatnonzero(ACGT == alt[pos])[0]) + 1) % 4]
            elif kind == 1:
                alt = np.concatenate([alt[:pos], ACGT[rng.integers(0, 4, int(rng.integers(1, 9)))], alt[pos:]])
            else:
                alt = np.concatenate([alt[:pos], alt[pos + int(rng.integers(1, 9)):]])
        reads = []
        for j in range(n_reads):
            hap = alt if (nvar and j % 2) else ref
            ln = min(read_len, len(hap))
            st = int(rng.integers(0, len(hap) - ln + 1))
            b = hap[st:st + ln].copy()
            bad = np.flatnonzero(rng.random(ln) < err)
            b[bad] = ACGT[rng.integers(0, 4, len(bad))]
            q = np.full(ln, ord("I"), np.uint8)
            if rng.random() < 0.1:
                q[int(rng.integers(0, ln))] = ord("#")
            reads.append((b.tobytes(), q.tobytes()))
        out.append(dict(ref=ref.tobytes(), reads=reads))
    return out


def traced(prep, reps):
    """Per-phase milliseconds from the library's own HC_ASM_TRACE line (stderr)."""
    rows = []
    os.environ["HC_ASM_TRACE"] = "1"
    try:
        for _ in range(reps):
            with tempfile.TemporaryFile() as tmp:
                sys.stderr.flush()
                saved = os.dup(2)
                os.dup2(tmp.fileno(), 2)
                try:
                    prep.free(prep.run())
                finally:
                    os.dup2(saved, 2)
                    os.close(saved)
                tmp.seek(0)
                line = [ln for ln in tmp.read().decode().splitlines() if ln.startswith("[hc_asm]")][-1]
            marks = dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in line.split()[1:])
            rows.append(marks)
    finally:
        del os.environ["HC_ASM_TRACE"]
    names = ["layout", "upload", "graph", "readback", "paths"]
    out, prev = {}, None
    for n in names:
        out[n] = round(statistics.median(r[n] - (r[prev] if prev else 0.0) for r in rows), 3)
        prev = n
    out["total_traced"] = round(statistics.median(r["paths"] for r in rows), 3)
    for n in ("walk_share", "slowest_region_ms", "its_walk_ms"):   # from the device's own clock
        if all(n in r for r in rows):
            out[n] = round(statistics.median(r[n] for r in rows), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=512)
    ap.add_argument("--window", type=int, default=415)
    ap.add_argument("--reads", type=int, default=415)
    ap.add_argument("--read-len", type=int, default=101)
    ap.add_argument("--err", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asm_timing.json"))
    a = ap.parse_args()
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    regs = build(a.regions, a.window, a.reads, a.read_len, err=a.err)
    prep = hcasm.Prepared(regs)
    h = prep.run()   # warm-up, and what the regions produce
    recs = hcasm.records(h, prep.n)
    prep.free(h)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h = prep.run()
        ts.append((time.perf_counter() - t0) * 1e3)
        prep.free(h)
    phases = traced(prep, a.trace_reps)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True,
                                text=True, check=True).stdout.strip()
    except Exception:
        commit = bid.get("git")
    ks = sorted({r["kmer_size"] for r in recs})
    res = dict(workload=dict(regions=a.regions, window=a.window, reads=a.reads, read_len=a.read_len, err=a.err,
                             read_bases=sum(len(b) for r in regs for b, _ in r["reads"])),
               reps=a.reps, statistic="median of reps after one warm-up call, wall clock around the C call, ms",
               assemble_ms=round(statistics.median(ts), 3), assemble_min_max_ms=[round(min(ts), 3), round(max(ts), 3)],
               phases_ms=phases, trace_reps=a.trace_reps,
               results=dict(status_counts=[sum(r["status"] == s for r in recs) for s in (0, 1, 2)],
                            kmer_size_counts={str(k): sum(r["kmer_size"] == k for r in recs) for k in ks},
                            haplotypes=sum(len(r["haps"]) for r in recs), paths=sum(r["n_paths"] for r in recs)),
               device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"]), commit=commit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
