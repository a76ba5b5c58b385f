#!/usr/bin/env python3
"""Times hc_contig_call against its two halves, on one generated contig of 512
windows (125 440 bases): reads of 101 bases, all "101M", sampled from the
reference and from a haplotype with one SNP per window origin; the number of
reads that begin at a position is Poisson with mean --per-position (1.7: a
depth of about 170, some 82 % of the positions hold a read). The file is
unsorted.

  contig_call_ms   (a) hc_contig_call: SAM text and reference in, VCF text out
  sam_parse_ms     (b) hc_sam_parse alone on the same text
  call_windows_ms  (c) hc_call_windows alone on the windows (a) sent, the
                   structs built outside the timed region: what the parent
                   commit can do, once its caller has parsed, bucketed and picked
  overhead_ms      (a) - ((b) + (c)), of the medians

Each figure: median, min and max of --reps calls after a warm-up call, wall
clock around the C call; every call ends in its own device synchronise. phases:
the HC_CONTIG_TRACE=1 and HC_SAM_TRACE=1 lines of --trace-reps further calls of
(a); their marks are milliseconds since the call began (the traces add
synchronisations, so their totals are not figure (a)).

Writes one JSON file with the figures, what the contig produced, the device and
the commit. Reads nothing outside the repository.
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

import hccall   # noqa: E402
import hccontig   # noqa: E402
import hcphmm   # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def generate(windows, region, read_len, per_position, seed):
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
    rows = ["@HD\tVN:1.6\tSO:unsorted", f"@SQ\tSN:chrT\tLN:{n}"]
    cigar = f"{read_len}M"
    for k, (s, w) in enumerate(zip(starts.tolist(), which.tolist())):
        q = (k * 37) % 4096
        rows.append(f"r{k}\t{99 if k % 2 else 147}\tchrT\t{s + 1}\t60\t{cigar}\t=\t{s + 200}\t300\t"
                    f"{srcs[w][s:s + read_len]}\t{quals[q:q + read_len]}")
    return ref.tobytes(), ("\n".join(rows) + "\n").encode(), int((counts > 0).sum())


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
    """Median of every name=value of the library's trace lines (stderr), per prefix; of a name a
    line repeats (one mark per batch) the last counts."""
    rows = {p: [] for p in prefixes}
    envs = ("HC_CONTIG_TRACE", "HC_SAM_TRACE")
    for env in envs:
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
        for env in envs:
            del os.environ[env]
    return {p: {k: round(statistics.median(r[k] for r in rs), 3) for k in rs[0]} for p, rs in rows.items()}


def chain_windows(text, ref, res):
    """The windows (a) sent, as hccall takes them."""
    recs, pool = res["sam"]["records"], res["sam"]["pool"]
    out = []
    for w in res["windows"]:
        if not w["picked"]:
            continue
        reads = []
        for k in w["picked"]:
            r = recs[k]
            reads.append(dict(flag=int(r["flag"]), mapq=int(r["mapq"]), pos=int(r["pos"]),
                              cigar=pool[int(r["cigar"]):int(r["cigar"]) + int(r["n_cigar"])],
                              mate_same=int(r["mate_same_contig"]), seq_len=int(r["seq_len"]),
                              bases=hccontig.seq(text, r), quals=hccontig.qual(text, r)))
        out.append(dict(ref=ref[w["padded_begin"]:w["padded_begin"] + w["ref_len"]], padded_begin=w["padded_begin"],
                        padded_end=w["padded_end"], origin_begin=w["origin_begin"],
                        origin_end=min(w["origin_end"], len(ref)), reads=reads))
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contig_timing.json"))
    a = ap.parse_args()
    import torch
    bid = hcphmm.ensure_built()
    hcphmm.init(0)
    ref, text, held = generate(a.windows, a.region, a.read_len, a.per_position, a.seed)

    # (a), and what the contig produces (the warm-up call)
    call = hccontig.Prepared(text, "chrT", ref, a.region, a.padding, seed=a.seed)
    h = call.run()
    res = hccontig.results(h)
    call.free(h)
    t_contig = timed(lambda: call.free(call.run()), a.reps)

    # (b)
    L = hccontig.lib()

    def parse():
        import ctypes as C
        hh = C.c_void_p()
        hccontig._check(L.hc_sam_parse(text, len(text), C.byref(hh)))
        L.hc_sam_result_free(hh)
    parse()
    t_parse = timed(parse, a.reps)

    # (c)
    chain = hccall.Prepared(chain_windows(text, ref, res))
    flags = hccall.flags_of()
    hc = chain.run(flags)
    cres = hccall.results(hc, chain.n)
    chain.free(hc)
    t_chain = timed(lambda: chain.free(chain.run(flags)), a.reps)
    sent = [k for k, w in enumerate(res["windows"]) if w["picked"]]
    same = ([w["status"] for w in cres["windows"]] == [res["windows"][k]["status"] for k in sent]
            and len(cres["sites"]) == len(res["sites"]))

    phases = traced(lambda: call.free(call.run()), a.trace_reps, ["[hc_contig]", "[hc_sam]"])
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True,
                                text=True, check=True).stdout.strip()
    except Exception:
        commit = bid.get("git")
    status = [w["status"] for w in res["windows"]]
    picks = [len(w["picked"]) for w in res["windows"]]
    n_lines = text.count(b"\n")
    out = dict(workload=dict(windows=a.windows, region=a.region, padding=a.padding, contig_bases=len(ref),
                             read_len=a.read_len, reads_per_position=a.per_position,
                             depth=round((n_lines - 2) * a.read_len / len(ref), 1), lines=n_lines, text_bytes=len(text),
                             records=int(len(res["sam"]["records"])), positions_with_reads=held,
                             picked_reads_per_window=dict(mean=round(statistics.mean(picks), 1), min=min(picks),
                                                          max=max(picks)), seed=a.seed),
               reps=a.reps, statistic="median, min, max of reps after one warm-up call, wall clock around the C call, ms",
               contig_call_ms=stats(t_contig), sam_parse_ms=stats(t_parse), call_windows_ms=stats(t_chain),
               overhead_ms=round(statistics.median(t_contig) - statistics.median(t_parse) - statistics.median(t_chain), 3),
               phases=phases, trace_reps=a.trace_reps,
               results=dict(status_counts=[status.count(s) for s in (0, 1, 2)], sites=len(res["sites"]),
                            emitted=sum(s["status"] == 0 for s in res["sites"]), vcf_bytes=len(res["vcf"]),
                            surviving_reads=sum(len(w["reads"]) for w in res["windows"]),
                            chain_alone_gives_the_same_statuses_and_site_count=bool(same)),
               device=torch.cuda.get_device_name(0), library=dict(kernel=bid["kernel"], lib=bid["lib"]), commit=commit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
