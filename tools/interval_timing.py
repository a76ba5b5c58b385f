#!/usr/bin/env python3
"""Times the interval calls (include/hc_intervals.h) against the plain calls on
the same reads: the one-contig shape of genome_timing.py (512 windows, reads of
101 bases, about 213 000 of them as 52 MB of SAM text), coordinate-sorted, as
SAM text and as BAM written by tests/bam_cases.to_bam at level 6 in members of
65 280 and of 4 096 bytes. The intervals cover 1/16 of the windows: in one run
of 32 consecutive windows, and in 8 scattered runs of 4.

Timed, in turn in one process:

  sam_plain                  hc_genome_call
  sam_one_run, sam_8_runs    hc_genome_call_intervals
  bam_plain                  hc_bam_genome_call, per member size
  bam_one_run, bam_8_runs    hc_bam_genome_call_intervals without an index, per member size
  bai_one_run, bai_8_runs    the same with the file's index (tests/bai_writer.py), per member size;
                             `index_stats`: the chunks, members, bytes uploaded and records framed

Each figure: median, min and max of --reps calls after a warm-up call, wall
clock around the C calls; `phases` is the HC_GENOME_TRACE=1 line of --trace-reps
further calls (marks in ms since the call began; the trace adds
synchronisations) and what each phase took; `vcf_lines` counts the lines of the
VCF text, and `vcf_is_the_plain_calls_inside` says that they are the plain
call's lines that begin inside the intervals. Writes one JSON file. Reads
nothing outside the repository.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bai_writer as BW   # noqa: E402
import bam_cases as BC   # noqa: E402
import hcbam   # noqa: E402
import hcgenome   # noqa: E402
import hcintervals   # noqa: E402
import hcphmm   # noqa: E402
from bam_timing import BAM_PHASES, SAM_PHASES, traced, vcf_of   # noqa: E402
from contig_timing import stats, timed   # noqa: E402
from genome_timing import generate   # noqa: E402


def with_scope(phases):
    at = phases.index("resolve") + 1
    return phases[:at] + ("scope",) + phases[at:]


INDEXED_PHASES = ("header", "index", "upload", "inflate", "crc", "frame", "decode", "readback") + with_scope(SAM_PHASES)[1:]


def index_stats(p):
    h = p.run()
    nc, nm, up, nr = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    hcintervals.lib().hc_bam_genome_result_index(h, C.byref(nc), C.byref(nm), C.byref(up), C.byref(nr))
    p.free(h)
    return dict(chunks=nc.value, members=nm.value, bytes_up=up.value, records=nr.value)


def sorted_by_position(text):
    lines = text.decode("latin-1").split("\n")
    head = [ln for ln in lines if ln.startswith("@")]
    body = [ln for ln in lines if ln and not ln.startswith("@")]
    body.sort(key=lambda ln: int(ln.split("\t")[3]))   # stable: file order within a position
    return "".join(ln + "\n" for ln in head + body).encode("latin-1")


def inside(vcf, intervals):
    return [ln for ln in vcf.split(b"\n")[4:-1] if any(b <= int(ln.split(b"\t")[1]) - 1 < e for _, b, e in intervals)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--region", type=int, default=245)
    ap.add_argument("--padding", type=int, default=85)
    ap.add_argument("--read-len", type=int, default=101)
    ap.add_argument("--per-position", type=float, default=1.7)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--member-sizes", type=int, nargs="*", default=[65280, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interval_timing.json"))
    a = ap.parse_args()
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    table, text, _ = generate(a.windows, 1, a.region, a.read_len, a.per_position, a.seed)
    text = sorted_by_position(text)
    n_asked = a.windows // 16
    one = [(0, (a.windows // 2 - n_asked // 2) * a.region, (a.windows // 2 + n_asked // 2) * a.region)]
    step, run = a.windows // 8, n_asked // 8
    eight = [(0, (k * step + step // 2) * a.region, (k * step + step // 2 + run) * a.region) for k in range(8)]
    kw = dict(region_size=a.region, padding_size=a.padding, seed=a.seed)

    calls = [("sam_plain", hcgenome.Prepared(text, table, **kw), SAM_PHASES, None),
             ("sam_one_run", hcintervals.Prepared(text, table, one, **kw), with_scope(SAM_PHASES), one),
             ("sam_8_runs", hcintervals.Prepared(text, table, eight, **kw), with_scope(SAM_PHASES), eight)]
    files = {}
    for size in a.member_sizes:
        t0 = time.perf_counter()
        bam = BC.to_bam(text, [(n, len(r)) for n, r in table], member_size=size, level=6)
        files[str(size)] = dict(bam_bytes=len(bam), members=len(BC.members(bam)))
        print(f"members of {size}: written in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        bai = BW.build(bam)
        files[str(size)]["bai_bytes"] = len(bai)
        calls += [(f"bam_plain_{size}", hcbam.Prepared(bam, table, **kw), BAM_PHASES, None),
                  (f"bam_one_run_{size}", hcintervals.PreparedBam(bam, table, one, **kw), with_scope(BAM_PHASES), one),
                  (f"bam_8_runs_{size}", hcintervals.PreparedBam(bam, table, eight, **kw), with_scope(BAM_PHASES), eight),
                  (f"bai_one_run_{size}", hcintervals.PreparedBam(bam, table, one, index=bai, **kw), INDEXED_PHASES, one),
                  (f"bai_8_runs_{size}", hcintervals.PreparedBam(bam, table, eight, index=bai, **kw), INDEXED_PHASES, eight)]

    vcfs = {name: vcf_of(p) for name, p, _, _ in calls}   # the warm-up of each
    times = {name: [] for name, _, _, _ in calls}
    for _ in range(a.reps):
        for name, p, _, _ in calls:
            times[name] += timed(lambda: p.free(p.run()), 1)
    result = {}
    for name, p, phases, intervals in calls:
        row = dict(call_ms=stats(times[name]), vcf_lines=vcfs[name].count(b"\n") - 4,
                   phases=traced(lambda: p.free(p.run()), a.trace_reps, phases))
        if intervals is not None:
            row["vcf_is_the_plain_calls_inside"] = bool(vcfs[name].split(b"\n")[4:-1] == inside(vcfs["sam_plain"], intervals))
            plain = "sam_plain" if name.startswith("sam") else "bam_plain_" + name.rsplit("_", 1)[1]
            row["over_plain"] = round(row["call_ms"]["median"] / result[plain]["call_ms"]["median"], 3)
            if name.startswith("bai"):
                row["index_stats"] = index_stats(p)
        else:
            row["vcf_equals_sam_plain"] = bool(vcfs[name] == vcfs["sam_plain"])
        result[name] = row
    out = dict(workload=dict(region=a.region, padding=a.padding, read_len=a.read_len, reads_per_position=a.per_position,
                             seed=a.seed, windows=a.windows, contigs=1, sam_bytes=len(text),
                             records=text.count(b"\n") - text.count(b"\n@") - 1, sorted_by="POS, file order within a position",
                             asked_windows=n_asked, one_run=one, eight_runs=eight, files=files,
                             bam="tests/bam_cases.to_bam, level 6",
                             batch_windows=os.environ.get("HC_CONTIG_BATCH_WINDOWS", "512")),
               reps=a.reps, trace_reps=a.trace_reps,
               statistic="median, min, max of reps calls, all calls in turn, after one warm-up call of each, wall clock "
                         "around the C calls, ms; phases: median of trace_reps traced calls",
               calls=result, device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
