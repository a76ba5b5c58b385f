#!/usr/bin/env python3
"""Times hc_bam_genome_call against hc_genome_call on the same reads: the
one-contig and the 64-contig shape of genome_timing.py (512 windows, reads of
101 bases, about 213 000 of them as 52 MB of SAM text), written as BAM by
tests/bam_cases.to_bam at level 6 in members of 65 280 bytes, against the text
sam_of(bam) that the BAM call stands in for.

Per shape:

  bam_call_ms, sam_call_ms   hc_bam_genome_call(bam) and hc_genome_call(sam_of(bam)),
                             in turn in one process, each with its own min-max spread
  phases                     the HC_GENOME_TRACE=1 line of --trace-reps further calls
                             of each: marks (ms since the call began; the trace adds
                             synchronisations) and what each phase took
  vcf_equal                  the two VCF texts are the same bytes

And once, on the one-contig file: hc_bgzf_inflate alone in GB/s of inflated
bytes, beside zlib.decompress over the same members on one host thread and on 16
(zlib releases the interpreter lock).

Each figure: median, min and max of --reps calls after a warm-up call, wall
clock around the C calls. Writes one JSON file. Reads nothing outside the
repository.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bam_cases as BC   # noqa: E402
import hcbam   # noqa: E402
import hcgenome   # noqa: E402
import hcphmm   # noqa: E402
from contig_timing import stats, timed   # noqa: E402
from genome_timing import generate   # noqa: E402

SAM_PHASES = ("parse", "resolve", "buckets", "picks", "structs", "chain", "vcf")
BAM_PHASES = ("upload", "inflate", "crc", "frame", "decode", "readback") + SAM_PHASES[1:]


def traced(fn, reps, phases):
    rows = []
    os.environ["HC_GENOME_TRACE"] = "1"
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
                line = [ln for ln in tmp.read().decode().splitlines() if ln.startswith("[hc_genome]")][-1]
            rows.append(dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in line.split()[1:] if kv != "front=bam"))
    finally:
        del os.environ["HC_GENOME_TRACE"]
    marks = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]}
    took, before = {}, 0.0
    for p in phases:
        if p in marks:
            took[p] = round(marks[p] - before, 3)
            before = marks[p]
    return dict(marks=marks, took_ms=took)


def vcf_of(p):
    h = p.run()
    t_, n_ = C.c_void_p(), C.c_int64()
    hcgenome.lib().hc_genome_result_vcf(h, C.byref(t_), C.byref(n_), None, None)
    v = C.string_at(t_, n_.value)
    p.free(h)
    return v


def shape(n_contigs, a):
    table, text, _ = generate(a.windows, n_contigs, a.region, a.read_len, a.per_position, a.seed)
    bam = BC.to_bam(text, [(n, len(r)) for n, r in table], member_size=65280, level=6)
    sam = BC.sam_of(bam)
    pb = hcbam.Prepared(bam, table, a.region, a.padding, seed=a.seed)
    ps = hcgenome.Prepared(sam, table, a.region, a.padding, seed=a.seed)
    vb, vs = vcf_of(pb), vcf_of(ps)   # the warm-up of each, and the bytes both must give
    tb, ts = [], []
    for _ in range(a.reps):
        tb += timed(lambda: pb.free(pb.run()), 1)
        ts += timed(lambda: ps.free(ps.run()), 1)
    sb, ss = stats(tb), stats(ts)
    out = dict(contigs=n_contigs, bam_bytes=len(bam), sam_bytes=len(sam), members=len(BC.members(bam)),
               records=sam.count(b"\n") - sam.count(b"\n@") - 1, vcf_bytes=len(vb), vcf_equal=bool(vb == vs),
               bam_call_ms=sb, sam_call_ms=ss, bam_minus_sam_ms=round(sb["median"] - ss["median"], 3),
               bam_spread_ms=round(sb["max"] - sb["min"], 3), sam_spread_ms=round(ss["max"] - ss["min"], 3),
               bam_median_inside_sam_min_max=bool(ss["min"] <= sb["median"] <= ss["max"]),
               bam_over_sam=round(sb["median"] / ss["median"], 3),
               bam_phases=traced(lambda: pb.free(pb.run()), a.trace_reps, BAM_PHASES),
               sam_phases=traced(lambda: ps.free(ps.run()), a.trace_reps, SAM_PHASES))
    return out, bam


def inflate_alone(bam, a):
    L = hcbam.lib()

    def device():
        h = C.c_void_p()
        assert L.hc_bgzf_inflate(bam, len(bam), C.byref(h)) == 0
        L.hc_bgzf_result_free(h)
    device()
    streams = [m[1] for m in BC.members(bam)]
    n = sum(m[3] for m in BC.members(bam))

    def host(threads):
        if threads == 1:
            for s in streams:
                zlib.decompress(s, -15)
        else:
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(lambda s: zlib.decompress(s, -15), streams, chunksize=8))
    out = dict(inflated_bytes=n, members=len(streams))
    for name, fn in (("hc_bgzf_inflate", device), ("zlib_1_thread", lambda: host(1)), ("zlib_16_threads", lambda: host(16))):
        ts = timed(fn, a.reps)
        out[name] = dict(ms=stats(ts), gb_per_s=round(n / statistics.median(ts) / 1e6, 3))
    os.environ["HC_BAM_TRACE"] = "1"
    try:
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                device()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            line = [ln for ln in tmp.read().decode().splitlines() if ln.startswith("[hc_bam]")][-1]
        out["hc_bgzf_inflate_trace_marks_ms"] = dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in line.split()[1:])
    finally:
        del os.environ["HC_BAM_TRACE"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--cuts", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--region", type=int, default=245)
    ap.add_argument("--padding", type=int, default=85)
    ap.add_argument("--read-len", type=int, default=101)
    ap.add_argument("--per-position", type=float, default=1.7)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_timing.json"))
    a = ap.parse_args()
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    shapes, first = {}, None
    for n in a.cuts:
        t0 = time.perf_counter()
        shapes[f"cut_{n}"], bam = shape(n, a)
        first = bam if first is None else first
        print(f"cut_{n}: done in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    out = dict(workload=dict(region=a.region, padding=a.padding, read_len=a.read_len, reads_per_position=a.per_position,
                             seed=a.seed, windows=a.windows, bam="tests/bam_cases.to_bam, level 6, members of 65280 bytes",
                             batch_windows=os.environ.get("HC_CONTIG_BATCH_WINDOWS", "512")),
               reps=a.reps, trace_reps=a.trace_reps,
               statistic="median, min, max of reps calls, BAM and SAM in turn, after one warm-up call of each, wall clock "
                         "around the C calls, ms; phases: median of trace_reps traced calls",
               shapes=shapes, inflate_alone=inflate_alone(first, a), device=torch.cuda.get_device_name(0),
               library=dict(kernel=bid["kernel"], lib=bid["lib"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
