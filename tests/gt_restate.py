"""Python restatement of Genetyper::assign_genotype_likelihoods' bookkeeping
(reference genotyper/genotyper.hpp:35-243,369-399), written from its semantics
with dicts, sorted() and bytes comparison. The arithmetic is the existing
GTOracle.site. Returns one record per in-origin site in the layout of
hcgt.call_regions."""
import re

import numpy as np

EMITTED, HOM_REF, LOW_QUALITY_HET, TOO_MANY_ALLELES = 0, 1, 2, 3
MAX_ALLELES = 7
U64 = 1 << 64


def events_of(ref, padded_begin, hap):
    """{begin: (begin, end, REF, ALT)}; the first event at a begin stays."""
    ev = {}
    ref_pos, hap_pos = hap["begin"], 0
    bases = hap["bases"]
    for n, op in re.findall(r"(\d+)(.)", hap["cigar"]):
        n = int(n)
        if op == "M":
            for o in range(n):
                if ref[ref_pos + o] != bases[hap_pos + o]:
                    b = padded_begin + ref_pos + o
                    ev.setdefault(b, (b, b + 1, ref[ref_pos + o:ref_pos + o + 1], bases[hap_pos + o:hap_pos + o + 1]))
            ref_pos += n
            hap_pos += n
        elif op == "I":
            if ref_pos > 0:
                b = padded_begin + ref_pos - 1
                anchor = ref[ref_pos - 1:ref_pos]
                ev.setdefault(b, (b, b + 1, anchor, anchor + bases[hap_pos:hap_pos + n]))
            hap_pos += n
        elif op == "D":
            if ref_pos > 0:
                b = padded_begin + ref_pos - 1
                ev.setdefault(b, (b, b + n + 1, ref[ref_pos - 1:ref_pos + n], ref[ref_pos - 1:ref_pos]))
            ref_pos += n
        elif op == "S":
            hap_pos += n
        else:
            raise ValueError("unsupported CIGAR operator")
    return ev


def call_region(region, oracle, index=0):
    ref, pb = region["ref"], region["padded_begin"]
    maps = [events_of(ref, pb, h) for h in region["haps"]]
    L = np.ascontiguousarray(region["L"], np.float64).reshape(len(region["read_begin"]), len(maps))
    out = []
    for begin in sorted({b for m in maps for b in m}):
        if not region["origin_begin"] <= begin < region["origin_end"]:
            continue
        overlapping = [[e for b, e in sorted(m.items()) if b <= begin < e[1]] for m in maps]
        site_ref = ref[begin - pb:begin - pb + 1]
        events = {e if e[0] == begin else (begin, begin + 1, site_ref, b"*") for evs in overlapping for e in evs}
        ref_allele = max((e[2] for e in events), key=len)
        loc_end = max(e[1] for e in events)

        def compatible(e):
            if e[2] == ref_allele or e[3] == b"*":
                return e[3]
            return e[3] + ref_allele[len(e[2]):]

        alleles = [ref_allele] + sorted({compatible(e) for e in events})
        rec = dict(region=index, begin=begin, loc_end=loc_end)
        if len(alleles) > MAX_ALLELES:
            rec.update(status=TOO_MANY_ALLELES, n_alleles=MAX_ALLELES + 1, alleles=[], hap_allele=np.zeros(0, np.int32),
                       keep=np.zeros(0, np.int32), genotype_likelihoods=np.zeros(0), genotype_index=-1, a1=-1,
                       a2=-1, genotype_quality=-1)
            out.append(rec)
            continue
        hap_allele = np.zeros(len(maps), np.int32)
        for h, evs in enumerate(overlapping):
            hits = [alleles.index(compatible(e)) if e[0] == begin else alleles.index(b"*") for e in evs]
            hap_allele[h] = max(hits, default=0)
        # begin < 2: the reference's begin - 2 wraps and Interval's constructor throws
        # (interval.hpp:26-31,82-83); the library cuts the window at the contig's first base
        lo, hi = max(begin - 2, 0), (loc_end + 2) % U64
        keep = np.array([r for r, (rb, re_) in enumerate(zip(region["read_begin"], region["read_end"]))
                         if int(rb) % U64 < hi and lo < int(re_) % U64], np.int32)
        gl, gi, gq = oracle.site(L, keep, hap_allele, len(alleles))
        pairs = [(a1, a2) for a1 in range(len(alleles)) for a2 in range(a1, len(alleles))]
        a1, a2 = pairs[gi]
        status = HOM_REF if gi == 0 else LOW_QUALITY_HET if a1 == 0 and gq < 50 else EMITTED
        rec.update(status=status, n_alleles=len(alleles), alleles=alleles, hap_allele=hap_allele, keep=keep,
                   genotype_likelihoods=np.asarray(gl, np.float64), genotype_index=int(gi), a1=a1, a2=a2,
                   genotype_quality=int(gq))
        out.append(rec)
    return out


def call_regions(regions, oracle):
    return [rec for k, r in enumerate(regions) for rec in call_region(r, oracle, k)]


def same_record(a, b):
    """Every field; likelihoods as bits."""
    for key in ("region", "status", "begin", "loc_end", "n_alleles", "genotype_index", "a1", "a2", "genotype_quality"):
        if a[key] != b[key]:
            return f"{key}: {a[key]} != {b[key]}"
    if list(a["alleles"]) != list(b["alleles"]):
        return f"alleles: {a['alleles']} != {b['alleles']}"
    for key in ("hap_allele", "keep"):
        if not np.array_equal(np.asarray(a[key], np.int32), np.asarray(b[key], np.int32)):
            return f"{key}: {a[key]} != {b[key]}"
    x = np.ascontiguousarray(a["genotype_likelihoods"], np.float64).view(np.uint64)
    y = np.ascontiguousarray(b["genotype_likelihoods"], np.float64).view(np.uint64)
    if not np.array_equal(x, y):
        return f"genotype_likelihoods: {a['genotype_likelihoods']} != {b['genotype_likelihoods']}"
    return None


def assert_same(got, exp):
    assert len(got) == len(exp), f"{len(got)} sites, expected {len(exp)}"
    for k, (g, e) in enumerate(zip(got, exp)):
        why = same_record(g, e)
        assert why is None, f"site {k} (region {e['region']}, begin {e['begin']}): {why}"
