#!/usr/bin/env python3
"""Times hc_genome_call against one hc_contig_call per contig, on the generated
contig of contig_timing.py (512 windows, 125 440 bases, reads of 101 bases,
Poisson 1.7 reads per position, unsorted) as one contig and cut into 8 and into
64 contigs of equal length, and on 1 000 contigs of one window each (245 000
bases generated the same way). A read that would hang over the end of its piece
is left out, so the cut shapes hold a few reads fewer (the counts are in the
output).

Per shape:

  genome_call_ms   (a) hc_genome_call: the whole text and the table in, one VCF out
  contig_calls_ms  (b) what the parent commit offers: one hc_contig_call per
                   contig, on texts filtered by RNAME beforehand; the filtering
                   is not timed, which favours (b)
  phases           the HC_GENOME_TRACE=1 line of --trace-reps further calls of (a):
                   the marks (ms since the call began; the trace adds
                   synchronisations) and what each phase took

For the one-contig shape (b) is hc_contig_call on the same text; the output
sets (a) - (b) against the min-max spread of (b)'s calls.

Each figure: median, min and max of --reps calls after a warm-up call, wall
clock around the C calls. Writes one JSON file. Reads nothing outside the
repository.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hccontig   # noqa: E402
import hcgenome   # noqa: E402
import hcphmm   # noqa: E402
from contig_timing import ACGT, stats, timed   # noqa: E402

PHASES = ("parse", "resolve", "buckets", "picks", "structs", "chain", "vcf")


def generate(windows, n_contigs, region, read_len, per_position, seed):
    """contig_timing.generate's bases and reads, cut into n_contigs pieces of
    equal length: ([(name, ref)], the whole text, per contig its own text)."""
    rng = np.random.default_rng(seed)
    n = windows * region
    ref = ACGT[rng.integers(0, 4, n)]
    hap = ref.copy()
    snps = np.arange(windows) * region + rng.integers(40, region - 40, windows)
    hap[snps] = ACGT[(np.searchsorted(ACGT, ref[snps]) + rng.integers(1, 4, windows)) % 4]
    counts = rng.poisson(per_position, n - read_len + 1)
    starts = np.repeat(np.arange(n - read_len + 1), counts)
    rng.shuffle(starts)
    which = rng.random(len(starts)) < 0.5
    quals = rng.integers(ord("F"), ord("J") + 1, 4096 + read_len).astype(np.uint8).tobytes().decode()
    srcs = (ref.tobytes().decode(), hap.tobytes().decode())
    piece = n // n_contigs
    assert piece * n_contigs == n and piece % region == 0
    names = [f"chr{c + 1}" for c in range(n_contigs)]
    header = ["@HD\tVN:1.6\tSO:unsorted"] + [f"@SQ\tSN:{nm}\tLN:{piece}" for nm in names]
    rows, per = list(header), [list(header) for _ in names]
    cigar = f"{read_len}M"
    for k, (s, w) in enumerate(zip(starts.tolist(), which.tolist())):
        c, at = divmod(s, piece)
        if at + read_len > piece:
            continue
        q = (k * 37) % 4096
        row = (f"r{k}\t{99 if k % 2 else 147}\t{names[c]}\t{at + 1}\t60\t{cigar}\t=\t{at + 200}\t300\t"
               f"{srcs[w][s:s + read_len]}\t{quals[q:q + read_len]}")
        rows.append(row)
        per[c].append(row)
    whole = ref.tobytes()
    table = [(nm, whole[c * piece:(c + 1) * piece]) for c, nm in enumerate(names)]
    return table, ("\n".join(rows) + "\n").encode(), [("\n".join(r) + "\n").encode() for r in per]


def traced(fn, reps):
    """Median of every name=value of the [hc_genome] trace line; of a name the line repeats the last counts."""
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
            rows.append(dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in line.split()[1:]))
    finally:
        del os.environ["HC_GENOME_TRACE"]
    marks = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]}
    took, before = {}, 0.0
    for p in PHASES:
        if p in marks:
            took[p] = round(marks[p] - before, 3)
            before = marks[p]
    return dict(marks=marks, took_ms=took)


def shape(windows, n_contigs, a):
    table, text, texts = generate(windows, n_contigs, a.region, a.read_len, a.per_position, a.seed)
    g = hcgenome.Prepared(text, table, a.region, a.padding, seed=a.seed)
    h = g.run()
    res = hcgenome.results(h, [n for n, _ in table])
    g.free(h)
    t_genome = timed(lambda: g.free(g.run()), a.reps)

    calls = [hccontig.Prepared(t, n, r, a.region, a.padding, seed=a.seed) for (n, r), t in zip(table, texts)]
    vcf = b""
    for c in calls:   # the warm-up, and the lines (a) must have
        hc = c.run()
        t_, n_ = C.c_void_p(), C.c_int64()
        hccontig.lib().hc_contig_result_vcf(hc, C.byref(t_), C.byref(n_), None)
        v = C.string_at(t_, n_.value)
        c.free(hc)
        vcf += v if not vcf else v.split(b"\n", 4)[4]   # the four header lines once

    def all_contigs():
        for c in calls:
            c.free(c.run())
    t_contigs = timed(all_contigs, a.reps)
    status = [w["status"] for w in res["windows"]]
    sent = sum(1 for w in res["windows"] if w["picked"])
    out = dict(contigs=n_contigs, windows=len(res["windows"]), contig_bases=len(table[0][1]), text_bytes=len(text),
               records=int(len(res["sam"]["records"])), sent_windows=sent,
               status_counts=[status.count(s) for s in (0, 1, 2)],
               emitted=sum(s["status"] == 0 for s in res["sites"]), vcf_bytes=len(res["vcf"]),
               genome_vcf_equals_the_contig_calls_lines=bool(res["vcf"] == vcf),
               genome_call_ms=stats(t_genome), contig_calls_ms=stats(t_contigs),
               genome_over_contig_calls=round(statistics.median(t_genome) / statistics.median(t_contigs), 3),
               phases=traced(lambda: g.free(g.run()), a.trace_reps))
    if n_contigs == 1:
        diff = statistics.median(t_genome) - statistics.median(t_contigs)
        spread = max(t_contigs) - min(t_contigs)
        out["one_contig"] = dict(genome_minus_contig_ms=round(diff, 3), contig_call_spread_ms=round(spread, 3),
                                 difference_exceeds_the_spread=bool(abs(diff) > spread))
    return out


def both_modes(table, text, a, sparse=False):
    """Dense and sorted in turn on one text and table."""
    modes = {m: hcgenome.Prepared(text, table, a.region, a.padding, seed=a.seed, sorted_buckets=(m == "sorted"))
             for m in ("dense", "sorted")}
    vcf, n_windows, n_records = {}, 0, 0
    for m, g in modes.items():   # the warm-up, and the bytes both must give
        h = g.run()
        t_, n_, w_ = C.c_void_p(), C.c_int64(), C.c_int32()
        hcgenome.lib().hc_genome_result_vcf(h, C.byref(t_), C.byref(n_), C.byref(w_), None)
        r_ = C.c_int32()
        hcgenome.lib().hc_genome_result_sam(h, None, None, C.byref(r_), None, None, None)
        vcf[m], n_windows, n_records = C.string_at(t_, n_.value), w_.value, r_.value
        g.free(h)
    ts = {m: [] for m in modes}
    for _ in range(a.reps):
        for m, g in modes.items():
            ts[m] += timed(lambda: g.free(g.run()), 1)
    out = dict(contigs=len(table), windows=n_windows, table_bases=sum(len(r) for _, r in table), text_bytes=len(text),
               records=n_records, vcf_bytes=len(vcf["dense"]), sorted_vcf_equals_dense=bool(vcf["dense"] == vcf["sorted"]))
    for m, g in modes.items():
        tr = traced(lambda: g.free(g.run()), a.trace_reps)
        out[m] = dict(genome_call_ms=stats(ts[m]), buckets_ms=tr["took_ms"]["buckets"], picks_ms=tr["took_ms"]["picks"],
                      tile_bytes=int(tr["marks"]["tile_bytes"]), sort_passes=int(tr["marks"]["sort_passes"]))
    d, s = out["dense"]["genome_call_ms"], out["sorted"]["genome_call_ms"]
    out["sorted_minus_dense_ms"] = round(s["median"] - d["median"], 3)
    out["dense_spread_ms"] = round(d["max"] - d["min"], 3)
    out["sorted_median_inside_dense_min_max"] = bool(d["min"] <= s["median"] <= d["max"])
    if sparse:
        out["dense_over_sorted"] = round(d["median"] / s["median"], 3)
    return out


def buckets_main(a):
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    shapes = {}
    wanted = lambda name: not a.only or name in a.only   # noqa: E731
    for n in a.cuts:
        if wanted(f"cut_{n}"):
            table, text, _ = generate(a.windows, n, a.region, a.read_len, a.per_position, a.seed)
            shapes[f"cut_{n}"] = both_modes(table, text, a)
            print(f"cut_{n}: done", file=sys.stderr, flush=True)
    name = f"one_window_x{a.small_contigs}"
    if a.small_contigs and wanted(name):
        table, text, _ = generate(a.small_contigs, a.small_contigs, a.region, a.read_len, a.per_position, a.seed)
        shapes[name] = both_modes(table, text, a)
    name = f"sparse_filler_2p{a.filler_bits}"
    if a.filler_bits and wanted(name):
        table, text, _ = generate(a.windows, 1, a.region, a.read_len, a.per_position, a.seed)
        shapes[name] = both_modes([("chrFill", b"A" * (1 << a.filler_bits))] + table, text, a, sparse=True)
    out = dict(workload=dict(region=a.region, padding=a.padding, read_len=a.read_len, reads_per_position=a.per_position,
                             seed=a.seed, batch_windows=os.environ.get("HC_CONTIG_BATCH_WINDOWS", "512")),
               reps=a.reps, trace_reps=a.trace_reps,
               statistic="median, min, max of reps calls per mode, dense and sorted in turn, after one warm-up call of each, "
                         "wall clock around the C calls, ms; phases: median of trace_reps traced calls",
               shapes=shapes, device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"]))
    write(a.out, out)


def write(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--cuts", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--small-contigs", type=int, default=1000, help="contigs of one window each (0: leave the shape out)")
    ap.add_argument("--region", type=int, default=245)
    ap.add_argument("--padding", type=int, default=85)
    ap.add_argument("--read-len", type=int, default=101)
    ap.add_argument("--per-position", type=float, default=1.7)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--buckets", action="store_true", help="dense against sorted buckets, in turn")
    ap.add_argument("--filler-bits", type=int, default=28, help="--buckets: the sparse shape's filler (0: leave it out)")
    ap.add_argument("--only", nargs="*", default=[], help="--buckets: the shapes to run")
    ap.add_argument("--merge", nargs="*", default=[], help="files of --buckets runs whose shapes go into --out")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "genome_sorted_timing.json" if a.buckets or a.merge else "genome_timing.json")
    if a.merge:
        parts = [json.load(open(f)) for f in a.merge]
        for p in parts[1:]:
            assert p["library"] == parts[0]["library"] and p["workload"] == parts[0]["workload"]
            parts[0]["shapes"].update(p["shapes"])
        return write(a.out, parts[0])
    if a.buckets:
        return buckets_main(a)
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    shapes = {}
    for n in a.cuts:
        shapes[f"cut_{n}"] = shape(a.windows, n, a)
        print(f"cut_{n}: done", file=sys.stderr, flush=True)
    if a.small_contigs:
        shapes[f"one_window_x{a.small_contigs}"] = shape(a.small_contigs, a.small_contigs, a)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True,
                                text=True, check=True).stdout.strip()
    except Exception:
        commit = bid.get("git")
    out = dict(workload=dict(region=a.region, padding=a.padding, read_len=a.read_len, reads_per_position=a.per_position,
                             seed=a.seed, batch_windows=os.environ.get("HC_CONTIG_BATCH_WINDOWS", "512")),
               reps=a.reps, trace_reps=a.trace_reps,
               statistic="median, min, max of reps after one warm-up call, wall clock around the C calls, ms",
               shapes=shapes, device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"]),
               commit=commit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
