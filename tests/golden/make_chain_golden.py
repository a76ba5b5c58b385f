"""Generate the fixture of the reference pins.

    make -C oracle oracle ref && python tests/golden/make_chain_golden.py

Writes tests/golden/chain_golden.npz: per stage (parse, prepare, align,
likelihoods, normalize, genotype, chain) one array `<stage>` of UTF-8 JSON
bytes holding [{name, input, output}]: the inputs of tests/pin_cases.py and what
the REFERENCE does with them, through its own headers compiled in place
(oracle/ref_chain_driver.cpp -> oracle/_ref/libref_chain.so). Data only:
doubles are stored as their 64 bits, an input on which the reference throws as
{"threw": true}. The file is the same bytes on every run (fixed member dates).

The generator refuses a fixture in which some stage's cases all throw, and one
that lacks an edge the pins are there for (see check())."""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in ("oracle", "gatk-haplotypecaller-cpp17_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import oracle  # noqa: E402
import pin_cases as P  # noqa: E402

OUT = os.path.join(HERE, "chain_golden.npz")
MAX_BYTES = os.path.getsize(os.path.join(HERE, "pairhmm_golden.npz"))


def cases_of(stage, gt_oracle):
    return dict(parse=P.parse_cases, prepare=P.prepare_cases, align=P.align_cases, likelihoods=P.likelihood_cases,
                normalize=P.normalize_cases, genotype=lambda: P.genotype_cases(gt_oracle), chain=P.chain_cases)[stage]()


def check(stage, rows):
    """The edges a stage's cases are there for, seen in what the reference did."""
    outs = {r["name"]: r["output"] for r in rows}
    done = [o for o in outs.values() if not o["threw"]]
    assert done, f"{stage}: the reference threw on every case"
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), f"{stage}: duplicate case names"
    if stage == "parse":
        assert outs["err_pos_plus"]["fail"] == 0 and outs["err_pos_plus"]["POS"] == 1   # libstdc++ takes "+1"
        assert outs["err_flag_overflow"]["fail"] == 1
        assert any(o["fail"] for o in done) and any(not o["fail"] for o in done)
    if stage == "prepare":
        reasons = {r["reason"] for o in done for r in o["reads"]}
        assert reasons == {0, 1, 2, 3, 4, 5}, reasons
        kept = [len(r["SEQ"]) for o in done for r in o["reads"] if not r["left"]]
        assert 10 in kept and min(kept) == 10
    if stage == "align":
        first = {o["cigar"].lstrip("0123456789")[0] for o in done}
        last = {o["cigar"][-1] for o in done}
        assert {"S", "M"} <= first and {"S", "M"} <= last, (first, last)
        assert any("I" in o["cigar"] for o in done) and any("D" in o["cigar"] for o in done)
        assert outs["equal_2_mismatches"]["cigar"] == "80M" and outs["equal_3_mismatches"]["threw"] is False
        assert any(o["offset"] > 0 for o in done)
    if stage == "likelihoods":
        assert len(outs["rescued_and_all_filtered"]["kept"]) == 0
        assert any(0 < len(o["kept"]) < o["raw"].shape[0] for o in done)
        capped = outs["capped"]
        assert not P.same_bits(capped["raw"][capped["kept"]], capped["L"])
    if stage == "normalize":
        n = len(outs["on_threshold"]["kept"])
        assert n and len(outs["below_threshold"]["kept"]) == 0 and len(outs["above_threshold"]["kept"]) == n
        assert len(outs["every_read_filtered"]["kept"]) == 0
    if stage == "genotype":
        sites = [s for o in done for s in o["sites"]]
        assert any(s["threw"] for s in sites) and any(o["whole_call_threw"] for o in done)
        assert {s["begin"] for s in sites if s["threw"]} <= {0, 1}
        ok = [s for s in sites if not s["threw"]]
        assert {7, 8} <= {len(s["alleles"]) for s in ok}
        assert any(b"*" in s["alleles"] for s in ok)
        assert any(len(s["keep"]) == 0 for s in ok if "keep" in s)
        assert any(np.isneginf(s["genotype_likelihoods"]).any() for s in ok if "keep" in s)
        assert sum(len(o["variants"]) for o in done) >= 10
        assert sum(k.startswith("quality_on_") for k in outs) >= 3, "no quality on .5 found"
    if stage == "chain":
        assert {o["outcome"] for o in done} == {0, 1, 2}
        assert sum(len(o["variants"]) for o in done) >= 4


def build():
    ref = oracle.ChainReference()
    gt_oracle = oracle.GTOracle()
    blobs = {}
    for stage in P.STAGES:
        rows = [dict(name=name, input=x, output=P.reference_output(stage, ref, x)) for name, x in cases_of(stage, gt_oracle)]
        check(stage, rows)
        blobs[stage] = json.dumps(P.encode(rows), sort_keys=True, separators=(",", ":")).encode()
        threw = sum(r["output"]["threw"] for r in rows)
        print(f"{stage}: {len(rows)} cases, the reference threw on {threw}, {len(blobs[stage])} bytes of JSON")
    return blobs


def write(blobs, path):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for stage in P.STAGES:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.frombuffer(blobs[stage], np.uint8), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(stage + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED, compresslevel=9)


def main():
    write(build(), OUT)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, f"{size} bytes: larger than the largest committed fixture ({MAX_BYTES})"
    print(f"wrote {OUT}: {size} bytes")


if __name__ == "__main__":
    main()
