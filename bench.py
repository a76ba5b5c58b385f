#!/usr/bin/env python3
"""PairHMM throughput bench (GCUPS) for the MI355X engine.

    python bench.py [--gpus N --steps K --warmup W --workload S2] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run sets up the batch, warms up, times the K steps and prints the
result line (with --dump-outputs DIR it also writes the last timed step's
results there). --full adds everything else this file measures and checks:
the end-to-end call path, the CPU baselines and their parity checks, the
secondary configs (S1, S1w, S4, shards, region calls, Smith-Waterman, the
genotyper) and the detail file; --no-cpu and --no-extra trim a --full run.

Workload (BASELINE.json configs[2] / configs[3]): the seeded synthetic WGS-mix
batch S2 — 1 000 000 independent (read, hap) pairs, H ~ U[100, 500],
R ~ U[50, min(250, H)], 1 % substitutions, Phred U[10, 40] (+33), GOP 'I',
GCP '+' (SURVEY.md §8(d)). One step = the whole device pass of the hot path
over that batch: fp32 anti-diagonal kernel, device-built rescue list, fp64
rescue kernel; with N > 1 the same batch is sharded by cells over the ranks
(strong scaling) and the step ends with the RCCL gather of the per-pair raw
results to rank 0 (configs[3]). Inputs are resident in HBM before timing.

Prints one JSON line (rank 0). `value` = total cells / max-over-ranks wall time
of the K timed steps. `roofline` prices the dominant kernel (fp32 PairHMM) by
its algorithmic work, 12 fp32 mul/add per cell, against the non-FMA fp32 VALU
rate; `cpu_baseline` times the reference's own AVX kernel (oracle/_ref) on the
host cores, same batch.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import statistics
import sys
import time

# The CPU baseline runs the reference's OpenMP kernel in this process; with the
# default wait policy its 16 threads keep spinning after each parallel region
# and take the host cores from the engine's planner threads in the host-path
# timings that follow (415 x 128 region 1.16 -> 1.23 ms, S2 end-to-end 1.55 ->
# 1.1-1.4 TCUPS). Passive waiting leaves the baseline itself unchanged (31.3
# GCUPS either way).
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd")
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402

VALU_PEAK_TOPS = 78.6      # 256 CU x 4 SIMD x 32 lanes x 2.4 GHz, one f32 mul/add per lane-cycle
FLOPS_PER_CELL = 12        # computeMXY: 8 mul + 4 add (avx-pairhmm-template.h:183-198)
HBM_PEAK_GBS = 8000.0


def algorithmic_bytes(b):
    """Per pair: read rows 5 B x R + hap H B + 8 B result."""
    return int(5 * b["R"].astype(np.int64).sum() + b["H"].astype(np.int64).sum() + 8 * len(b["R"]))


def cpu_baseline(batch, threads, reps, sample_desc):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    kind = "reference"
    try:
        lib = oracle.Reference()
    except FileNotFoundError:
        lib, kind = oracle.Oracle(), "port"
    import workloads as W
    cells = W.cells(batch)
    best = None
    res = None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = lib.pairs(batch, nthreads=threads)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return dict(value=cells / best / 1e9, unit="GCUPS", cores=threads, kind=kind,
                sample=sample_desc, seconds=round(best, 3)), res


def pmc_from_profiles(workload, cells, kernel_ms, world):
    """Counters of the dominant kernel from the committed PMC summary of this
    exact configuration (profiles/r*_pmc_<workload>.json, written by
    tools/profile_r03.sh + tools/profile_summary.py): used only when its kernel
    source hash (tools/kernel_src_hash.py) equals the tree's and it profiled the
    same cell count on one GPU; otherwise traffic is null. Reports HBM bytes per
    launch (2*FETCH_SIZE + WRITE_SIZE, gfx950 rule), LDS bank-conflict cycles,
    VALU lane-instructions per cell, the measured HBM rate traffic / kernel
    time, and the profile's own warm-average frac beside this run's."""
    if world != 1:
        return dict(traffic_note="PMC profiles are single-GPU; N>1 reports traffic null")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_src_hash import kernel_src_hash
    want = kernel_src_hash()
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_{workload}.json")))
    for path in reversed(cands):
        try:
            d = json.load(open(path))
            if d.get("kernel_src_hash") != want or int(d.get("cells", -1)) != int(cells):
                continue
            k = d["kernels"][d.get("fp32_kernel") or d["dominant_kernel"]]
            out = dict(traffic=int(d["hbm_bytes_per_launch"]), traffic_source=os.path.relpath(path, ROOT),
                       kernel_src_hash=want, profile_kernel_ms_warm=k.get("avg_ms_warm"),
                       profile_frac=d.get("frac_from_warm_avg"),
                       lds_bank_conflict_cycles=int(k.get("SQ_LDS_BANK_CONFLICT", 0)),
                       valu_lane_instr_per_cell=d.get("valu_lane_instr_per_cell"),
                       write_bytes_per_launch=d.get("write_bytes_per_launch"),
                       dominant_kernel=d.get("dominant_kernel"))
            if d.get("fp64_kernel") and d.get("rescued_cells"):
                k64 = d["kernels"][d["fp64_kernel"]]
                out["fp64_pmc"] = dict(kernel=d["fp64_kernel"], profile_kernel_ms_warm=k64.get("avg_ms_warm"),
                                       rescued_cells=d["rescued_cells"],
                                       profile_frac=d.get("fp64_frac_from_warm_avg"),
                                       valu_lane_instr_per_rescued_cell=d.get("fp64_valu_lane_instr_per_rescued_cell"),
                                       mean_resident_waves_per_busy_cycle=d.get(
                                           "fp64_mean_resident_waves_per_busy_cycle"))
            if kernel_ms > 0:
                out["hbm_measured_GBs"] = round(out["traffic"] / (kernel_ms * 1e-3) / 1e9, 2)
            return out
        except (OSError, KeyError, ValueError, TypeError):
            continue
    return dict(traffic_note=f"no committed PMC profile of this config with kernel source hash {want}")


def host_cpu():
    """CPUs this process may use and the CPU model. The share is the cgroup CPU
    quota when one is set (the GPU box grants 16 CPUs of a 256-CPU machine;
    affinity and os.cpu_count() show the whole machine), else the affinity set."""
    cores = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            cores = max(1, min(cores, int(int(q) // int(per))))
    except (OSError, ValueError):
        pass
    model = "?"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return cores, model


SW_OPS_PER_CELL = 22       # MAIN_CODE int32 vector ops per cell (PairWiseSW.h:4-38)
INT32_VALU_PEAK_TOPS = 78.6   # 256 CU x 4 SIMD-32 x 32 lanes x 2.4 GHz (wave64 issues over 2 cycles; no packed int32 ops)
# gfx950 issues v_add/v_sub/logic at that rate but v_max, v_alignbit, compares
# and DPP moves at half of it (profiles/r02_op_rate_ubench.jsonl). The DP
# kernel's fast path issues 9 full-rate + 11 half-rate instructions per cell:
# 31 full-rate issue slots, so its own instruction-mix ceiling is
# 256 x 4 x 32 x 2.4e9 / 31 cells/s.
SW_MIX_SLOTS_PER_CELL = 31
SW_MIX_CEILING_TCUPS = 256 * 4 * 32 * 2.4e9 / SW_MIX_SLOTS_PER_CELL / 1e12


def sw_secondary(no_cpu: bool):
    """Smith-Waterman on W2: 512 region windows (300-600
    bp) x 128 haplotypes, NEW_SW_PARAMETERS, SOFTCLIP, all-match shortcut — the
    graph_wrapper.hpp:232-240 loop for 512 regions in one device pass. Device
    pass timed with HIP events; the reference aligner (oracle/_ref, 1 thread,
    as the reference calls it) on the first 16 regions, checked for identical
    offsets and CIGARs."""
    import hcsw
    import sw_workloads as SWW
    hcsw.init(-1)   # the device the PairHMM engine was initialised on
    b = SWW.config("W2")
    bt = hcsw.Batch(b)
    for _ in range(2):
        bt.run()
    bt.stats()
    for _ in range(5):
        bt.run()
    st = bt.stats()
    off, cig = bt.results()
    bt.close()
    cells = st["cells"]
    tcups = cells / (st["dp_ms"] * 1e-3) / 1e12
    ent = dict(workload="W2", pairs=st["n_pairs"], shortcut_pairs=st["n_shortcut"], dp_cells=cells,
               dp_kernel_ms=round(st["dp_ms"], 3), trace_kernel_ms=round(st["trace_ms"], 3),
               device_pass_ms=round(st["run_ms"], 3), gcups=round(cells / (st["run_ms"] * 1e-3) / 1e9, 1),
               roofline=dict(bound="valu-int32", achieved=round(tcups * SW_OPS_PER_CELL, 2),
                             peak=INT32_VALU_PEAK_TOPS, unit="Top/s",
                             frac=round(tcups * SW_OPS_PER_CELL / INT32_VALU_PEAK_TOPS, 4),
                             note=f"{SW_OPS_PER_CELL} int32 ops/cell x DP cells / sw_dp_kernel time",
                             mix_ceiling_tcups=round(SW_MIX_CEILING_TCUPS, 3),
                             frac_of_mix_ceiling=round(tcups / SW_MIX_CEILING_TCUPS, 4),
                             mix_note=f"{SW_MIX_SLOTS_PER_CELL} full-rate issue slots per cell (9 full-rate + 11 "
                                      "half-rate VALU); includes the one-row skew and partial-stripe cells"))
    # one region through the host API (the real per-region call shape)
    one = SWW.config("W1")
    hcsw.align_flat(one)
    t0 = time.perf_counter()
    for _ in range(5):
        hcsw.align_flat(one)
    ent["region_415x128_call_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    if not no_cpu:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle
        kind = "reference"
        try:
            ref = oracle.SWReference()
        except FileNotFoundError:
            ref, kind = oracle.SWOracle(), "port"
        nreg = 16
        idx = np.arange(nreg * 128)
        sub = SWW.subset(b, idx)
        t0 = time.perf_counter()
        r_off, r_cig = ref.batch(sub)
        dt = time.perf_counter() - t0
        same = np.array_equal(r_off, off[idx]) and r_cig == [cig[k] for k in idx]
        ent["cpu_baseline"] = dict(value=round(SWW.dp_cells(sub) / dt / 1e9, 3), unit="GCUPS", cores=1, kind=kind,
                                   sample=f"first {nreg} regions of W2 ({len(idx)} pairs), IntelSWAligner::align "
                                          f"semantics, 1 thread", seconds=round(dt, 3))
        ent["parity_vs_cpu_reference"] = "identical" if same else "MISMATCH"
        t0 = time.perf_counter()
        ref.batch(one)
        ent["region_415x128_cpu_reference_1core_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    return ent


def gt_secondary(no_cpu: bool):
    """Genotyper numeric core: 512 regions (415 reads x
    32 haps, normalised log10 likelihoods) x 16 variant sites, one call of
    hc_gt_genotype_sites with host buffers (the matrices' upload included); the
    oracle (C restatement, 1 thread) on the same sites beside it, compared bit
    for bit."""
    import hcgt
    import gt_workloads as GW
    mats, sites = GW.sites(n_regions=512, sites_per_region=16, reads=(415, 415), haps=(32, 32), seed=63)
    prep = hcgt.Prepared(mats, sites)
    prep.run()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        prep.run()
    dt = (time.perf_counter() - t0) / reps
    got = prep.results()
    ent = dict(regions=len(mats), sites=len(sites), call_ms=round(dt * 1e3, 3),
               note="host matrices in, per-site genotype likelihoods / GT / GQ out; 54 MB of likelihoods uploaded per call")
    if not no_cpu:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle
        orc = oracle.GTOracle()
        import ctypes as C
        _f, _i = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        args = []
        for s in sites:   # marshal first: time the C loop, not ctypes
            L = mats[s["m"]]
            A = s["n_alleles"]
            gl = np.zeros(A * (A + 1) // 2)
            gi, gq = C.c_int32(), C.c_int32()
            args.append(((L.ctypes.data_as(_f), L.shape[1], s["keep"].ctypes.data_as(_i), len(s["keep"]),
                          s["hap_allele"].ctypes.data_as(_i), A, gl.ctypes.data_as(_f), C.byref(gi), C.byref(gq)),
                         gl, gi, gq))
        fn = orc.lib.hco_gt_site
        t0 = time.perf_counter()
        for a, *_ in args:
            fn(*a)
        dc = time.perf_counter() - t0
        exp = [(gl, gi.value, gq.value) for _, gl, gi, gq in args]
        same = all(np.array_equal(g[0].view(np.uint64), e[0].view(np.uint64)) and g[1] == e[1] and g[2] == e[2]
                   for g, e in zip(got, exp))
        ent["cpu_baseline"] = dict(value=round(dc * 1e3, 1), unit="ms", cores=1, kind="port",
                                   sample="same sites, oracle/gt_oracle.c (genotyper.hpp is not buildable here)")
        ent["parity_vs_cpu_oracle"] = "bit-exact" if same else "MISMATCH"
    return ent


FP64_PEAK_TOPS = 39.3   # AMD MI355X FP64 vector 78.6 TFLOPS (FMA = 2) -> 39.3 T non-FMA op/s; the guide has no FP64 row
# fp64 cell on gfx950: 11 f64 mul/add (EQ path) at 2 issue
# slots + v_bfe and two v_bitop3 (the prior select) at 2 = 28 slots, against
# the 12 algorithmic f64 ops' 24: 0.857 of the fp64 peak before per-step
# overhead and skew.
FP64_MIX_CEILING = 0.857


def resident_pass(hcphmm, W, name, npairs, prof, batch=None):
    """One BASELINE config as a device-resident batch: 10 timed device passes
    (HIP events, back to back) after at least 5 untimed ones and 0.2 s of
    them: the GPU's clocks rise over the first tens of ms of work after an idle
    spell (rank 0's 125k-pair shard: 1.29 ms on the first pass of a sequence,
    1.18 ms on the tenth, tools/shard_state_probe.py), and the bench's other
    steps leave it idle between configs. S4 also prices its fp64 rescue pass
    (intel_pairhmm.hpp:137-139): 12 f64 ops per rescued cell / fp64 pass time
    vs the fp64 peak. `batch`: a given batch (a shard) instead of the config's."""
    b = W.config(name, npairs) if batch is None else batch
    bb = hcphmm.Batch(b)
    # Cold: the batch's first pass, alone, after the host-side steps before it
    # (the GPU idle, its clocks down): what a lone call sees, reported beside
    # the warm average of back-to-back passes (verdict round 4).
    bb.run()
    s0 = bb.stats()
    t0, k = time.perf_counter(), 0
    while k < 5 or time.perf_counter() - t0 < 0.2:
        bb.run()
        k += 1
        if k % 4 == 0:
            bb.stats()   # (synchronises: bounds the queued passes)
    bb.stats()
    for _ in range(10):
        bb.run()
    s2 = bb.stats()
    cells = W.cells(b)
    ent = dict(pairs=len(b["R"]), cells=cells, device_pass_ms=round(s2.run_ms, 4),
               device_pass_ms_cold=round(s0.run_ms, 4), kernel_ms_f32_cold=round(s0.kernel_ms_f32, 4),
               kernel_ms_f64_cold=round(s0.kernel_ms_f64, 4),
               gcups=round(cells / (s2.run_ms * 1e-3) / 1e9, 2),
               kernel_ms_f32=round(s2.kernel_ms_f32, 4),
               frac_f32_kernel=round(12 * cells / (s2.kernel_ms_f32 * 1e-3) / 78.6e12, 4)
               if s2.kernel_ms_f32 > 0 else None,
               kernel_ms_f64=round(s2.kernel_ms_f64, 4), rescued=int(s2.n_rescued),
               new_batch_device_ms=round(s2.run_ms + s2.pack_ms, 4))
    pmc = pmc_from_profiles(prof, cells, s2.kernel_ms_f32, 1)
    if "traffic" in pmc:
        ent["pmc"] = {k: pmc.get(k) for k in ("traffic", "traffic_source", "profile_kernel_ms_warm", "profile_frac",
                                              "hbm_measured_GBs", "valu_lane_instr_per_cell", "write_bytes_per_launch",
                                              "dominant_kernel", "fp64_pmc")}
    if s2.n_rescued:
        r = bb.results()
        m = r["rescued"].astype(bool)
        rc = int(np.dot(b["R"][m].astype(np.int64), b["H"][m].astype(np.int64)))
        ent["rescued_cells"] = rc
        # The whole pass against both peaks: the time the fp32 cells (12 ops
        # each at 78.6 T) and the rescued fp64 cells (12 at 39.3 T) take at
        # peak, over the device pass.
        t_peak = FLOPS_PER_CELL * cells / 78.6e12 + FLOPS_PER_CELL * rc / (FP64_PEAK_TOPS * 1e12)
        ent["roofline_pass"] = dict(bound="valu f32 + f64", time_at_peak_ms=round(t_peak * 1e3, 4),
                                    frac=round(t_peak * 1e3 / s2.run_ms, 4))
    if s2.n_rescued and s2.kernel_ms_f64 > 0:
        ach = FLOPS_PER_CELL * rc / (s2.kernel_ms_f64 * 1e-3) / 1e12
        ent["fp64_tcups"] = round(rc / (s2.kernel_ms_f64 * 1e-3) / 1e12, 3)
        frac = ach / FP64_PEAK_TOPS
        ent["roofline_f64"] = dict(bound="valu-f64", achieved=round(ach, 3), peak=FP64_PEAK_TOPS, unit="T op/s",
                                   frac=round(frac, 4), frac_of_mix_ceiling=round(frac / FP64_MIX_CEILING, 4),
                                   note="12 f64 mul/add per rescued cell / fp64 rescue pass (plan + kernels) time; "
                                        "peak = AMD spec FP64 vector 78.6 TFLOPS with FMA counted as 2; mix ceiling "
                                        f"{FP64_MIX_CEILING}: 24 issue slots of algorithmic work in 28 per cell "
                                        "(DESIGN.md §15)")
    bb.close()
    return ent


def end_to_end(hcphmm, W, batch, total_cells):
    """The real call path on the S2 batch: host buffers in, log10 likelihoods
    out (hc_phmm_pairs_flat: host planning + staging + H2D + device packing +
    kernels + D2H + host log10, the call cut into parts so the planning of part
    k+1 overlaps the device pass of part k). Median of 3 after a first call
    that sizes the workspaces."""
    n = len(batch["R"])
    outs = [hcphmm.result_arrays(n) for _ in range(2)]   # the caller's result buffers, reused
    for o in outs:
        for v in o.values():
            v.fill(0)   # touched once, as a caller's long-lived buffers are
    t0 = time.perf_counter()
    hcphmm.pairs(batch, outs[0])
    first = time.perf_counter() - t0
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        hcphmm.pairs(batch, outs[0])
        reps.append(time.perf_counter() - t0)
    e2e = float(np.median(reps))
    # Two calls in flight: submit the second before collecting the first (after
    # one such round that sizes the second set of workspaces).
    for j in [hcphmm.submit_pairs(batch, outs[0]), hcphmm.submit_pairs(batch, outs[1])]:
        j.collect()
    t0 = time.perf_counter()
    j1 = hcphmm.submit_pairs(batch, outs[0])
    j2 = hcphmm.submit_pairs(batch, outs[1])
    j1.collect()
    j2.collect()
    two = time.perf_counter() - t0
    return {"end_to_end_gcups": round(total_cells / e2e / 1e9, 2), "end_to_end_ms": round(e2e * 1e3, 2),
            "end_to_end_first_call_ms": round(first * 1e3, 2),
            "end_to_end_async_2calls_gcups": round(2 * total_cells / two / 1e9, 2),
            "end_to_end_note": "hc_phmm_pairs_flat on host buffers (host staging of nibble-packed records, H2D, "
                               "device packing + planning, kernels, D2H, host log10) into reused result "
                               "buffers, median of 5; async: two submit_pairs in flight"}


def region_calls(hcphmm, W, no_cpu):
    """One active region (415 reads x N haps, hap ~415 bp, read 150 bp), the
    call shape of IntelPairHMM::compute_likelihoods (haplotypecaller.hpp:103):
    host buffers in, doubles out. `call_ms` times the C call (median of 30; argument structs
    built once, as a C++ caller holds them); `python_call_ms` includes building
    them from Python bytes each time. Then 64 such regions (415 x 32) in one
    cross-region call, and the same 64 as a stream of 8 submits of 8 regions."""
    sec = {}
    for nh in (32, 128):
        reads, haps = W.region(415, nh)
        call = hcphmm.CrossCall(reads, haps)
        for _ in range(5):
            call()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        dt = statistics.median(ts)   # host-clock jitter on a shared box: median, mean beside it
        # cold: a call after 0.25 s of idle (the GPU's clocks down), median of 5
        tc = []
        for _ in range(5):
            time.sleep(0.25)
            t0 = time.perf_counter()
            call()
            tc.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for _ in range(5):
            hcphmm.cross(reads, haps)
        dpy = (time.perf_counter() - t0) / 5
        flat = W.region_flat(reads, haps)
        ent = dict(reads=len(reads), haps=nh, cells=W.cells(flat), call_ms=round(dt * 1e3, 3),
                   call_ms_cold=round(statistics.median(tc) * 1e3, 3),
                   call_ms_mean=round(sum(ts) / len(ts) * 1e3, 3), call_ms_min=round(min(ts) * 1e3, 3),
                   python_call_ms=round(dpy * 1e3, 3), gcups=round(W.cells(flat) / dt / 1e9, 2))
        if not no_cpu:
            c1, _ = cpu_baseline(flat, 1, 1, "same region, 1 thread")
            ent["cpu_reference_1core_ms"] = round(c1["seconds"] * 1e3, 1)
        sec[f"region_415x{nh}"] = ent
    regs = [W.region(415, 32, seed=1000 + k) for k in range(64)]
    rc = sum(W.cells(W.region_flat(r, h)) for r, h in regs)
    call = hcphmm.RegionsCall(regs)
    groups = [hcphmm.RegionsCall(regs[k:k + 8]) for k in range(0, 64, 8)]
    for _ in range(2):   # size the workspaces (several parts / jobs in flight)
        call()
        for j in [g.submit() for g in groups]:
            j.collect()
    t0 = time.perf_counter()
    call()
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    jobs = [g.submit() for g in groups]
    for j in jobs:
        j.collect()
    dj = time.perf_counter() - t0
    sec["regions_64x_415x32_one_call"] = dict(regions=len(regs), cells=rc, call_ms=round(dt * 1e3, 2),
                                               gcups=round(rc / dt / 1e9, 2),
                                               stream_8x8_submits_ms=round(dj * 1e3, 2),
                                               stream_gcups=round(rc / dj / 1e9, 2))
    return sec


def compact_line(out, detail_path):
    """The bench line: the contract's keys, the roofline and CPU baseline, and
    the secondaries' headline figures (device pass / call times, fractions of
    peak); everything else is in the detail file (`detail`)."""
    rf = out["roofline"]
    line = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                "higher_is_better", "scaling", "vs_baseline", "dtype")}
    line["data"] = "synthetic (seeded generator, SURVEY 8d)"
    line["config"] = {k: out["config"][k] for k in ("pairs", "cells", "parallelism", "rescued_fp64")
                      if k in out["config"]}
    line["config"]["workload"] = out["config"]["workload"].replace("independent pairs", "pairs").replace(
        "1000000 ", "1M ")
    line["roofline"] = {k: rf.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel",
                                               "kernel_ms", "traffic_source")}
    if "cpu_baseline" in out:
        cb = out["cpu_baseline"]
        line["cpu_baseline"] = dict(value=round(cb["value"], 2), unit=cb["unit"], cores=cb["cores"], kind=cb["kind"],
                                    sample=f"full batch, {cb['cores']} threads, {cb.get('cpu_model', '?')[:24]}")
    for k in ("parity_vs_cpu_reference", "device_pass_ms", "kernel_ms_f64", "new_batch_device_ms",
              "end_to_end_gcups", "end_to_end_first_call_ms", "end_to_end_async_2calls_gcups",
              "multi_rank_check", "gather"):
        if k in out:
            line[k] = out[k]
    if "cpu_baseline_1core" in out:
        line["cpu_1core_gcups"] = round(out["cpu_baseline_1core"]["value"], 3)
    sec = out.get("secondary") or {}
    short = {}
    for k in ("S1", "S1w", "S1w1M", "S4", "S4_20k"):
        if k in sec:
            e = sec[k]
            v = dict(gcups=e.get("gcups"), pass_ms=e.get("device_pass_ms"), f32_frac=e.get("frac_f32_kernel"))
            if k in ("S1", "S1w", "S4"):   # one-round passes: a lone call's (cold) time beside
                v["cold_ms"] = e.get("device_pass_ms_cold")
            if e.get("roofline_f64"):
                v.update(f64_ms=e.get("kernel_ms_f64"), f64_frac=e["roofline_f64"]["frac"],
                         rescued=e.get("rescued"))
            short[k] = v
    for k in ("S2_shard_125k", "S2_shard_250k"):
        if k in sec:
            short[k] = dict(pass_ms=sec[k]["device_pass_ms"], eff=sec[k].get("implied_efficiency_vs_1gpu"))
    for k in ("region_415x32", "region_415x128"):
        if k in sec:
            short[k] = dict(call_ms=sec[k]["call_ms"], cold_ms=sec[k]["call_ms_cold"])
    if "regions_64x_415x32_one_call" in sec:
        e = sec["regions_64x_415x32_one_call"]
        short["regions_64"] = dict(call_ms=e["call_ms"], gcups=e["gcups"])
    if "smith_waterman" in sec:
        e = sec["smith_waterman"]
        short["sw"] = dict(pass_ms=e["device_pass_ms"], frac=e["roofline"]["frac"],
                           parity=e.get("parity_vs_cpu_reference"))
    if "genotyper" in sec:
        e = sec["genotyper"]
        short["gt"] = dict(call_ms=e["call_ms"], parity=e.get("parity_vs_cpu_oracle"))
    if short:
        line["secondary"] = short
    bid = out.get("build_id") or {}
    line["build"] = f"{bid.get('kernel')} {bid.get('git')}"
    line["detail"] = os.path.relpath(detail_path, ROOT) if detail_path else None
    return line


DUMP_MAX_BYTES = 64_000_000


def dump_outputs(path, arrays):
    """--dump-outputs: each per-pair result array as path/<name>.npy, float32 or
    float64 (the rescue flags as float32 0/1). A batch whose arrays pass
    DUMP_MAX_BYTES in all is written as a fixed, seeded sample of its pairs,
    with the sampled pair indices beside it (index.npy)."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, v.dtype if v.dtype in (np.float32, np.float64) else np.float32)
              for k, v in arrays.items()}
    n = len(next(iter(arrays.values())))
    per_pair = sum(v.itemsize for v in arrays.values())
    if n * per_pair > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // (per_pair + 8)
        idx = np.sort(np.random.default_rng(20).choice(n, keep, replace=False))
        arrays = {k: v[idx] for k, v in arrays.items()}
        arrays["index"] = idx.astype(np.float64)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="S2", choices=["S1", "S1w", "S2", "S4"])
    ap.add_argument("--pairs", type=int, default=None, help="override pair count")
    ap.add_argument("--shard-of", type=int, default=0,
                    help="run rank 0's shard of an N-way split of the batch (shard.shard_pairs), at one GPU")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = every core of this process's CPU set")
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also run the end-to-end call path, the CPU baselines and parity checks and the "
                         "secondary configs, and write the detail file (off: only the timed steps)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's results (raw_f32, raw_f64, rescued; batch order) "
                         "as DIR/<name>.npy")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip end-to-end and secondary configs")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (default); gloo only to rehearse N ranks on one GPU")
    ap.add_argument("--check", type=int, default=0,
                    help="rank 0 re-computes this many random pairs alone and compares them bit for bit "
                         "with the gathered multi-rank results")
    ap.add_argument("--check-out", default=None, help="with --check: save the reassembled results (npz)")
    ap.add_argument("--force-dist", action="store_true",
                    help="use the process group / gather path even at WORLD_SIZE=1 (tests of the RCCL path)")
    args = ap.parse_args()
    extra = args.full and not args.no_extra   # end-to-end and secondary configs
    cpu = args.full and not args.no_cpu       # CPU baselines and parity against them

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))

    import torch
    import torch.distributed as dist

    import hcphmm
    import shard
    import workloads as W

    ndev = torch.cuda.device_count()
    gpu = local % max(ndev, 1)   # several ranks per GPU only when rehearsing with gloo
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    gloo = args.dist_backend == "gloo"
    # --force-dist: the distributed path (process group, gathers, check) at one
    # rank, so a one-GPU box exercises the RCCL code the 8-GPU run uses.
    distributed = world > 1 or args.force_dist
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if gloo:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    # Refuse a stale binary: the library's compiled-in source hashes must be
    # this tree's (the bench line carries them as build_id).
    build_id = hcphmm.check_build_id()
    hcphmm.init(gpu)

    batch = W.config(args.workload, args.pairs)
    if args.shard_of > 1:   # one rank's share of configs[3], measured alone
        batch = W.subset(batch, shard.shard_pairs(batch["R"], batch["H"], args.shard_of)[0])
    n_total = len(batch["R"])
    total_cells = W.cells(batch)
    shards = shard.shard_pairs(batch["R"], batch["H"], world)
    mine = shards[rank]
    sub = batch if world == 1 else W.subset(batch, mine)
    my_cells = W.cells(sub)
    nmax = max(len(s) for s in shards)

    bt = hcphmm.Batch(sub)
    # Two output sets: with RCCL the gather of step k (on its own stream) runs
    # while step k + 1's device pass writes the other set.
    nsets = 2 if (distributed and not gloo) else 1
    outs = [(torch.zeros(nmax, dtype=torch.float32, device=dev), torch.zeros(nmax, dtype=torch.float64, device=dev),
             torch.zeros(nmax, dtype=torch.uint8, device=dev)) for _ in range(nsets)]
    raw32, raw64, flag = outs[0]
    bt.bind_outputs(raw32.data_ptr(), raw64.data_ptr(), flag.data_ptr())
    gdev = torch.device("cpu") if gloo else dev
    g32 = [torch.empty(nmax, dtype=torch.float32, device=gdev) for _ in range(world)] if (distributed and rank == 0) else None
    g64 = [torch.empty(nmax, dtype=torch.float64, device=gdev) for _ in range(world)] if (distributed and rank == 0) else None

    # The device pass runs on a created stream: the library enqueues on it (a
    # created stream's handle is non-zero; 0 would select the library's own
    # stream, unordered with torch's). The gather of a step's outputs waits for
    # that step's pass (event), and the pass that next writes the same output
    # set waits for that gather (event): RCCL over xGMI overlaps the next pass.
    stream = torch.cuda.Stream(device=dev)
    cstream = torch.cuda.Stream(device=dev) if nsets == 2 else stream
    ran_ev = [torch.cuda.Event() for _ in range(nsets)]
    gathered_ev = [None] * nsets
    nstep = [0]

    def step():
        k = nstep[0] % nsets
        nstep[0] += 1
        r32, r64, fl = outs[k]
        with torch.cuda.stream(stream):
            if gathered_ev[k] is not None:
                stream.wait_event(gathered_ev[k])
            if nsets == 2:
                bt.bind_outputs(r32.data_ptr(), r64.data_ptr(), fl.data_ptr())
            bt.run(stream.cuda_stream)
            ran_ev[k].record(stream)
        if distributed:
            with torch.cuda.stream(cstream):
                cstream.wait_event(ran_ev[k])
                s32, s64 = (r32.cpu(), r64.cpu()) if gloo else (r32, r64)
                dist.gather(s32, gather_list=g32, dst=0)   # RCCL gather over xGMI
                dist.gather(s64, gather_list=g64, dst=0)
                if nsets == 2:
                    ev = torch.cuda.Event()
                    ev.record(cstream)
                    gathered_ev[k] = ev

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    bt.stats()   # reset the kernel event log: the averages below cover the timed steps only
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    st = bt.stats()
    ms_step = elapsed / args.steps * 1e3
    value = total_cells * args.steps / elapsed / 1e9

    if args.dump_outputs and rank == 0:
        # What the last timed step handed its caller: the bound output set of
        # that step (one rank) or rank 0's gather buffers (every rank's shard),
        # put back in batch order.
        last = outs[(nstep[0] - 1) % nsets]
        if distributed:
            got = {"raw_f32": np.zeros(n_total, np.float32), "raw_f64": np.zeros(n_total, np.float64)}
            for r, sh in enumerate(shards):
                got["raw_f32"][sh] = g32[r][: len(sh)].cpu().numpy()
                got["raw_f64"][sh] = g64[r][: len(sh)].cpu().numpy()
        else:
            got = {k: t[:n_total].cpu().numpy() for k, t in zip(("raw_f32", "raw_f64", "rescued"), last)}
        dump_outputs(args.dump_outputs, got)

    # Dominant kernel: the fp32 PairHMM pass. Algorithmic work 12 ops/cell.
    k_ms = st.kernel_ms_f32
    achieved = FLOPS_PER_CELL * my_cells / (k_ms * 1e-3) / 1e12 if k_ms > 0 else 0.0
    prof_name = args.workload if args.pairs is None else f"{args.workload}_{args.pairs}"
    if args.shard_of > 1:
        prof_name = f"{args.workload}shard_{args.shard_of}"
    pmc = pmc_from_profiles(prof_name, my_cells, k_ms, world)
    roofline = dict(bound="valu", achieved=round(achieved, 3), peak=VALU_PEAK_TOPS, unit="TFLOP/s",
                    frac=round(achieved / VALU_PEAK_TOPS, 4), traffic=pmc.get("traffic"),
                    kernel=(("phmm_seg_kernel" if st.n_seg_waves > 0 else "phmm_lane_kernel")
                            if st.n_lane_pairs == st.n_pairs else "phmm_diag_kernel<float,16>"),
                    kernel_ms=round(k_ms, 4),
                    flops_per_cell=FLOPS_PER_CELL, cells_per_launch=my_cells,
                    hbm_algorithmic_GBs=round(algorithmic_bytes(sub) / (k_ms * 1e-3) / 1e9, 2) if k_ms > 0 else None,
                    hbm_measured_GBs=pmc.get("hbm_measured_GBs"), hbm_peak_GBs=HBM_PEAK_GBS,
                    lds_bank_conflict_cycles=pmc.get("lds_bank_conflict_cycles"),
                    valu_lane_instr_per_cell=pmc.get("valu_lane_instr_per_cell"),
                    traffic_source=pmc.get("traffic_source"), traffic_note=pmc.get("traffic_note"),
                    kernel_src_hash=build_id["tree_kernel"], lib_kernel_src_hash=build_id.get("kernel"),
                    profile_kernel_ms_warm=pmc.get("profile_kernel_ms_warm"), profile_frac=pmc.get("profile_frac"))

    out = {
        "metric": "PairHMM GCUPS (cell updates/s), fp32 pass + fp64 rescue",
        "value": round(value, 2), "unit": "GCUPS", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
        "scaling": "strong" if world > 1 else "strong", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic (seeded generator, SURVEY.md §8(d))",
        "config": {"workload": f"{args.workload}: {n_total} independent pairs"
                               + (", H~U[100,500], R~U[50,min(250,H)], 1% subst" if args.workload == "S2" else ""),
                   "pairs": n_total, "cells": total_cells, "parallelism": f"pair-shard x{world}",
                   "rescued_fp64": int(st.n_rescued) if world == 1 else None},
        "roofline": roofline,
        "kernel_ms_f64": round(st.kernel_ms_f64, 4),
        "device_pass_ms": round(st.run_ms, 4),
        # A batch seen for the first time also packs its rows and hap tables on
        # the device (once per batch, outside the resident-batch step above).
        "new_batch_device_ms": round(st.run_ms + st.pack_ms, 4),
        "pack_ms": round(st.pack_ms, 4),
        "upload_bytes": int(st.upload_bytes),
        "build_id": build_id,
    }

    # The real call path, timed before the CPU baseline's all-core run (which
    # leaves the host's caches and clocks in another state for a while).
    if rank == 0 and world == 1 and extra:
        out.update(end_to_end(hcphmm, W, batch, total_cells))

    cpu_res = None
    if rank == 0 and world == 1 and cpu:
        cores, model = host_cpu()
        thr = args.cpu_threads or cores
        cb, cpu_res = cpu_baseline(batch, thr, args.cpu_reps,
                                   f"the full {args.workload} batch ({n_total} pairs), {thr} OpenMP threads "
                                   f"(every CPU of this process's share), best of {args.cpu_reps}")
        cb.update(nproc=cores, cpu_model=model, machine_cpus=os.cpu_count())
        out["cpu_baseline"] = cb
        if extra:
            s1 = W.subset(batch, np.arange(min(n_total, 20_000)))
            c1, _ = cpu_baseline(s1, 1, 1, f"first {len(s1['R'])} pairs of {args.workload}, 1 thread "
                                           "(the reference as built: OpenMP compiled out)")
            out["cpu_baseline_1core"] = c1

    if rank == 0 and world == 1 and args.full:
        r = bt.results()
        out["config"]["rescued_fp64"] = int(r["rescued"].sum())
        m = r["rescued"].astype(bool)
        out["config"]["rescued_cells"] = int(np.dot(sub["R"][m].astype(np.int64), sub["H"][m].astype(np.int64)))
        if cpu_res is not None:
            same = all(np.array_equal(np.ascontiguousarray(r[k]).view(np.uint8),
                                      np.ascontiguousarray(cpu_res[k]).view(np.uint8))
                       for k in ("raw_f32", "rescued", "loglik"))
            out["parity_vs_cpu_reference"] = "bit-exact" if same else "MISMATCH"
    if rank == 0 and world == 1 and extra:
        sec = {}
        # S1w1M: the north star's 101x250 shape at a size that fills the chip
        # (S1/S1w are 10k-pair, latency-bound passes of < 0.15 ms).
        # S4_20k: the S4 shape at 20 000 pairs, a rescue pass large enough to
        # fill the chip with fp64 waves (S4 itself rescues ~2k pairs).
        for label, name, npairs in (("S1", "S1", None), ("S1w", "S1w", None), ("S1w1M", "S1w", 1_000_000),
                                    ("S4", "S4", None), ("S4_20k", "S4", 20_000)):
            sec[label] = resident_pass(hcphmm, W, name, npairs, name if npairs is None else f"{name}_{npairs}")
        # configs[3]'s per-rank work: rank 0's shard of the S2 batch at 8 and 4
        # ranks (shard.shard_pairs, the same cut bench.py makes at N > 1), so the
        # driver's 1-GPU run carries the per-rank cost of its 8-GPU curve.
        for label, nr in ((("S2_shard_125k", 8), ("S2_shard_250k", 4)) if args.workload == "S2" and not args.pairs
                          and not args.shard_of else ()):
            sh = W.subset(batch, shard.shard_pairs(batch["R"], batch["H"], nr)[0])
            sec[label] = resident_pass(hcphmm, W, "S2", None, f"S2shard_{nr}", batch=sh)
            sec[label]["per_rank_of"] = nr
            # warm: back-to-back steps, as the bench's own N-rank steps run;
            # cold: a rank's first pass after idle (the worst case)
            sec[label]["implied_efficiency_vs_1gpu"] = round(
                out["device_pass_ms"] / (nr * sec[label]["device_pass_ms"]), 4) if sec[label]["device_pass_ms"] else None
            sec[label]["implied_efficiency_vs_1gpu_cold"] = round(
                out["device_pass_ms"] / (nr * sec[label]["device_pass_ms_cold"]), 4) \
                if sec[label]["device_pass_ms_cold"] else None
        sec.update(region_calls(hcphmm, W, not cpu))
        sec["smith_waterman"] = sw_secondary(not cpu)
        sec["genotyper"] = gt_secondary(not cpu)
        out["secondary"] = sec
    if distributed:
        out["gather"] = (f"dist.gather ({'gloo, rehearsal' if gloo else 'RCCL'}) of raw_f32 + raw_f64 per step"
                         + ("" if gloo else ", on its own stream overlapping the next step's pass (two output sets)"))
    if args.check and distributed:
        # One more step into outputs poisoned with NaN on every rank (and in rank
        # 0's gather buffers): what is gathered must come from this very run.
        with torch.cuda.stream(stream):
            for r32, r64, _fl in outs:
                r32.fill_(float("nan"))
                r64.fill_(float("nan"))
            for g in (g32 or []) + (g64 or []):
                g.fill_(float("nan"))
        torch.cuda.synchronize()
        dist.barrier()
        step()
        torch.cuda.synchronize()
    if args.check and distributed and rank == 0:
        # Reassemble batch order from the gathered shards and compare a random
        # sample with a single-process run of the same pairs.
        full32 = np.zeros(n_total, np.float32)
        full64 = np.zeros(n_total, np.float64)
        for r, sh in enumerate(shards):
            full32[sh] = g32[r][: len(sh)].cpu().numpy()
            full64[sh] = g64[r][: len(sh)].cpu().numpy()
        idx = np.sort(np.random.default_rng(7).choice(n_total, min(args.check, n_total), replace=False))
        ref = hcphmm.pairs(W.subset(batch, idx))
        ok = (np.array_equal(full32[idx].view(np.uint32), ref["raw_f32"].view(np.uint32)) and
              np.array_equal(full64[idx].view(np.uint64), ref["raw_f64"].view(np.uint64)))
        ok = ok and not np.isnan(full32).any() and not np.isnan(full64).any()
        out["multi_rank_check"] = f"{len(idx)} pairs {'bit-exact' if ok else 'MISMATCH'}"
        if args.check_out:
            np.savez(args.check_out, raw_f32=full32, raw_f64=full64)
    bt.close()
    if rank == 0:
        # The whole record (every secondary's PMC summary, notes, baselines) goes
        # to a file; stdout carries one compact line (< 2 kB) that a driver's
        # output tail holds whole (verdict round 5, item 5).
        detail = os.environ.get("HC_BENCH_DETAIL", os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
        if not args.full:   # a plain run prints its line and writes no detail file
            detail = None
        try:
            if detail:
                os.makedirs(os.path.dirname(detail), exist_ok=True)
                with open(detail, "w") as f:
                    json.dump(out, f, indent=1)
        except OSError:
            detail = None
        print(json.dumps(compact_line(out, detail), separators=(",", ":")), flush=True)
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
