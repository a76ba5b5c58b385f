// Genotyper event bookkeeping on gfx950, ahead of gt_sites_kernel.
//
// Reference: src/haplotypecaller/genotyper/genotyper.hpp — process_cigar_for_
// initial_events (:35-111), set_events_for_haplotypes (:113-127), get_events_
// from_haplotypes / replace_span_dels / get_compatible_alleles (:129-193),
// get_allele_mapper / get_haplotype_mapper (:195-232), get_read_indices_to_keep
// (:234-243); Haplotype::get_overlapping_events (haplotype/haplotype.hpp:31-39).
//
// gt_plan_events_kernel  one wave per haplotype. The reference keeps a map keyed
//   by the event begin and emplaces in CIGAR order, so the first event at a
//   position wins: here every candidate does an LDS atomicMin of its run index
//   on its position, which gives the same winner whatever the lane timing. The
//   result is two position-indexed tables per haplotype (ascending begin by
//   construction): the run owning the event that begins at a position, and the
//   deletion run that covers a position from an earlier begin. Event begins
//   inside the origin are OR-ed into the region's position bitmap.
// gt_plan_scan_kernel    one wave: per region popcount of the bitmap, exclusive
//   prefix over the regions -> dense site numbering and the buffer totals.
// gt_plan_site_kernel    one wave per site: the k-th set bit of its region's
//   bitmap is its position; lanes gather the haplotypes' overlapping events,
//   the wave runs the small allele state machine uniformly (distinct alts by
//   kind, length and own bytes; bytewise order by a ballot compare), then lanes
//   write the haplotype -> allele map and the kept reads (ballot + prefix count)
//   and the GtSite record of the arithmetic kernel.
//
// An alt allele at a site with reference allele ref[p, p+R) is, by kind:
//   SNP   hap byte            + ref[p+1, p+R)
//   INS   ref[p] + len bytes  + ref[p+1, p+R)
//   DEL   ref[p]              + ref[p+len+1, p+R)
//   STAR  "*"
// so two alts are the same text iff kind, len and own bytes agree (the lengths
// R, R+len, R-len differ otherwise), and no tail needs comparing to find that.
#include "gt_plan_kernels.hpp"

#include <climits>

namespace hcgt {
namespace {

constexpr int kNoOwner = INT_MAX;

__global__ __launch_bounds__(64) void gt_plan_events_kernel(PlanArgs a)
{
    __shared__ int owner[kMaxRefLen + 1];
    __shared__ int cover[kMaxRefLen + 1];
    const int lane = threadIdx.x;
    const PlanHap H = a.haps[blockIdx.x];
    const PlanRegion R = a.regions[H.region];
    const uint8_t* ref = a.ref + R.ref_off;
    const uint8_t* hap = a.hap + H.base_off;
    const PlanRun* runs = a.runs + H.run_off;
    for (int p = lane; p < R.ref_len; p += 64) {
        owner[p] = kNoOwner;
        cover[p] = -1;
    }
    __syncthreads();
    for (int base = 0; base < H.n_runs; base += 64) {
        const int mine = base + lane;
        PlanRun r{0, kOpS, 0, 0};
        if (mine < H.n_runs) r = runs[mine];
        if ((r.op == kOpI || r.op == kOpD) && r.ref_pos > 0) atomicMin(&owner[r.ref_pos - 1], mine);
        const int cnt = min(64, H.n_runs - base);
        for (int j = 0; j < cnt; ++j) {
            if (__shfl(r.op, j) != kOpM) continue;
            const int len = __shfl(r.len, j), rp = __shfl(r.ref_pos, j), hp = __shfl(r.hap_pos, j);
            for (int o = lane; o < len; o += 64)
                if (ref[rp + o] != hap[hp + o]) atomicMin(&owner[rp + o], base + j);
        }
    }
    __syncthreads();
    // Deletions that own their begin cover the positions after it.
    for (int base = 0; base < H.n_runs; base += 64) {
        const int mine = base + lane;
        PlanRun r{0, kOpS, 0, 0};
        if (mine < H.n_runs) r = runs[mine];
        const bool del = r.op == kOpD && r.ref_pos > 0 && owner[r.ref_pos - 1] == mine;
        uint64_t todo = __ballot(del);
        while (todo) {
            const int j = __ffsll(static_cast<unsigned long long>(todo)) - 1;
            todo &= todo - 1;
            const int len = __shfl(r.len, j), rp = __shfl(r.ref_pos, j);
            for (int o = lane; o < len; o += 64) cover[rp + o] = base + j;
        }
    }
    __syncthreads();
    int16_t* ev = a.ev + H.tab_off;
    int16_t* span = a.span + H.tab_off;
    uint32_t* bitmap = a.bitmap + size_t(H.region) * kBitmapWords;
    for (int p = lane; p < R.ref_len; p += 64) {
        const int o = owner[p];
        ev[p] = o == kNoOwner ? int16_t(-1) : int16_t(o);
        span[p] = int16_t(cover[p]);
        const int64_t begin = R.padded_begin + p;
        if (o != kNoOwner && begin >= R.origin_begin && begin < R.origin_end)
            atomicOr(&bitmap[p >> 5], 1u << (p & 31));
    }
}

__device__ __forceinline__ int64_t wave_inclusive(int64_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

__global__ __launch_bounds__(64) void gt_plan_scan_kernel(PlanArgs a)
{
    const int lane = threadIdx.x;
    int64_t cs = 0, ck = 0, cm = 0;
    for (int r0 = 0; r0 < a.n_regions; r0 += 64) {
        const int r = r0 + lane;
        int64_t c = 0, nr = 0, nh = 0;
        if (r < a.n_regions) {
            for (int w = 0; w < kBitmapWords; ++w) c += __popc(a.bitmap[size_t(r) * kBitmapWords + w]);
            nr = a.regions[r].n_reads;
            nh = a.regions[r].n_haps;
        }
        const int64_t is = wave_inclusive(c, lane), ik = wave_inclusive(c * nr, lane), im = wave_inclusive(c * nh, lane);
        if (r < a.n_regions) {
            PlanBase b;
            b.site_base = int32_t(cs + is - c);
            b.n_sites = int32_t(c);
            b.map_base = int32_t(cm + im - c * nh);
            b.pad = 0;
            b.keep_base = ck + ik - c * nr;
            a.base[r] = b;
        }
        cs += __shfl(is, 63);
        ck += __shfl(ik, 63);
        cm += __shfl(im, 63);
    }
    if (lane == 0) {
        a.totals->n_sites = cs;
        a.totals->keep_cap = ck;
        a.totals->map_cap = cm;
    }
}

struct AltCtx {
    const uint8_t* ref;   // the region's window
    const uint8_t* hap;   // the haplotype pool
    int p, R;             // site position, reference allele length
};

__device__ __forceinline__ int alt_length(const AltCtx& c, int kind, int len)
{
    return kind == kAltStar ? 1 : kind == kAltSnp ? c.R : kind == kAltIns ? c.R + len : c.R - len;
}

__device__ __forceinline__ int alt_byte(const AltCtx& c, int kind, int len, int hp, int j)
{
    if (kind == kAltStar) return '*';
    if (kind == kAltSnp) return j == 0 ? c.hap[hp] : c.ref[c.p + j];
    if (kind == kAltIns) return j == 0 ? c.ref[c.p] : j <= len ? c.hap[hp + j - 1] : c.ref[c.p + j - len];
    return j == 0 ? c.ref[c.p] : c.ref[c.p + len + j];
}

// Wave-uniform: do the two candidates spell the same alt?
__device__ bool same_alt(const AltCtx& c, int lane, int k1, int l1, int h1, int k2, int l2, int h2)
{
    if (k1 != k2) return false;
    if (k1 == kAltStar) return true;
    if (k1 == kAltSnp) return c.hap[h1] == c.hap[h2];
    if (l1 != l2) return false;
    if (k1 == kAltDel) return true;
    bool diff = false;
    for (int j = lane; j < l1; j += 64) diff |= c.hap[h1 + j] != c.hap[h2 + j];
    return __ballot(diff) == 0;
}

// Wave-uniform std::string operator< on two distinct alts.
__device__ bool alt_less(const AltCtx& c, int lane, int k1, int l1, int h1, int k2, int l2, int h2)
{
    const int n1 = alt_length(c, k1, l1), n2 = alt_length(c, k2, l2);
    const int n = min(n1, n2);
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const bool diff = j < n && alt_byte(c, k1, l1, h1, j) != alt_byte(c, k2, l2, h2, j);
        const uint64_t m = __ballot(diff);
        if (m) {
            const int f = base + __ffsll(static_cast<unsigned long long>(m)) - 1;
            return alt_byte(c, k1, l1, h1, f) < alt_byte(c, k2, l2, h2, f);
        }
    }
    return n1 < n2;
}

__global__ __launch_bounds__(64) void gt_plan_site_kernel(PlanArgs a, int n_sites)
{
    __shared__ int s_kind[kMaxHaps], s_len[kMaxHaps], s_hp[kMaxHaps], s_id[kMaxHaps], s_cov[kMaxHaps];
    __shared__ int s_ak[kMaxAlleles], s_al[kMaxAlleles], s_ah[kMaxAlleles];
    const int lane = threadIdx.x;
    const int s = blockIdx.x;
    if (s >= n_sites) return;
    // The region holding dense site s: the last one whose first site is <= s.
    int lo = 0, hi = a.n_regions - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.base[mid].site_base <= s) lo = mid;
        else hi = mid - 1;
    }
    const int r = lo;
    const PlanRegion R = a.regions[r];
    const PlanBase B = a.base[r];
    const int k = s - B.site_base;
    // Its position: the k-th set bit of the region's bitmap.
    int p;
    {
        const uint32_t w = lane < kBitmapWords ? a.bitmap[size_t(r) * kBitmapWords + lane] : 0u;
        const int c = __popc(w);
        const int incl = int(wave_inclusive(c, lane));
        const uint64_t m = __ballot(incl - c <= k && k < incl);
        const int src = __ffsll(static_cast<unsigned long long>(m)) - 1;
        uint32_t ws = __shfl(w, src);
        for (int skip = k - __shfl(incl - c, src); skip > 0; --skip) ws &= ws - 1;
        p = src * 32 + __ffs(int(ws)) - 1;
    }
    const int nh = R.n_haps;
    AltCtx c{a.ref + R.ref_off, a.hap, p, 1};
    // Gather: each haplotype has at most one event beginning at p and at most
    // one earlier deletion covering p.
    int maxR = 1;
    for (int h = lane; h < nh; h += 64) {
        const PlanHap H = a.haps[R.hap0 + h];
        const int e = a.ev[H.tab_off + p];
        int kind = kAltNone, len = 0, hp = 0;
        if (e >= 0) {
            const PlanRun run = a.runs[H.run_off + e];
            if (run.op == kOpM) {
                hp = H.base_off + run.hap_pos + (p - run.ref_pos);
                kind = a.hap[hp] == '*' ? kAltStar : kAltSnp;
                len = 1;
            } else if (run.op == kOpI) {
                kind = kAltIns;
                len = run.len;
                hp = H.base_off + run.hap_pos;
            } else {
                kind = c.ref[p] == '*' ? kAltStar : kAltDel;
                len = run.len;
                maxR = max(maxR, run.len + 1);
            }
        }
        s_kind[h] = kind;
        s_len[h] = len;
        s_hp[h] = hp;
        s_id[h] = -1;
        s_cov[h] = a.span[H.tab_off + p] >= 0;
    }
    for (int d = 32; d > 0; d >>= 1) maxR = max(maxR, __shfl_xor(maxR, d));
    c.R = maxR;
    __syncthreads();
    // Distinct alts, every lane running the same steps on the same values.
    int n_alts = 0, star_id = -1;
    bool too_many = false;
    for (int h = 0; h < nh && !too_many; ++h) {
        for (int which = 0; which < 2; ++which) {
            int kind, len = 0, hp = 0;
            if (which == 0) {
                kind = s_kind[h];
                len = s_len[h];
                hp = s_hp[h];
            } else {
                kind = s_cov[h] ? kAltStar : kAltNone;
            }
            if (kind == kAltNone) continue;
            int id = -1;
            for (int q = 0; q < n_alts && id < 0; ++q)
                if (same_alt(c, lane, kind, len, hp, s_ak[q], s_al[q], s_ah[q])) id = q;
            if (id < 0) {
                if (n_alts == kMaxAlleles - 1) {   // a 7th distinct alt: the site is skipped anyway
                    too_many = true;
                    break;
                }
                id = n_alts++;
                s_ak[id] = kind;
                s_al[id] = len;
                s_ah[id] = hp;
            }
            if (kind == kAltStar) star_id = id;
            if (which == 0) s_id[h] = id;
        }
    }
    const int map_off = B.map_base + k * nh;
    const int64_t keep_off = B.keep_base + int64_t(k) * R.n_reads;
    SiteOut out{};
    out.region = r;
    out.pos = p;
    out.ref_len = c.R;
    out.keep_off = int32_t(keep_off);
    out.map_off = map_off;
    int n_keep = 0;
    if (too_many) {
        out.n_alleles = kMaxAlleles + 1;
        for (int h = lane; h < nh; h += 64) a.amap[map_off + h] = 0;
    } else {
        out.n_alleles = n_alts + 1;
        // std::set<std::string> order: rank = number of smaller alts, 4 bits each.
        uint32_t ranks = 0;
        for (int i = 0; i < n_alts; ++i)
            for (int j = i + 1; j < n_alts; ++j)
                ranks += 1u << (4 * (alt_less(c, lane, s_ak[i], s_al[i], s_ah[i], s_ak[j], s_al[j], s_ah[j]) ? j : i));
        auto rank_of = [ranks](int i) { return int((ranks >> (4 * i)) & 15u); };
        for (int i = 0; i < n_alts; ++i) out.alt[rank_of(i)] = AltDesc{s_ak[i], s_al[i], s_ah[i]};
        // get_index searches the allele list from the reference allele on, and
        // "*" can be the reference allele only where the window itself holds '*'.
        const int star_allele = star_id < 0 ? 0 : (c.R == 1 && c.ref[p] == '*') ? 0 : rank_of(star_id) + 1;
        for (int h = lane; h < nh; h += 64) {
            int v = 0;
            if (s_id[h] >= 0) v = s_kind[h] == kAltStar ? star_allele : rank_of(s_id[h]) + 1;
            if (s_cov[h]) v = max(v, star_allele);
            a.amap[map_off + h] = v;
        }
        // Interval::overlaps with the allele window widened by 2 on both sides and
        // cut at the contig's first base. For begin < 2 the reference's begin - 2
        // wraps and its Interval constructor throws (interval.hpp:26-31,82-83), so
        // there the window is ours to define: expand_within_contig as it is named.
        const uint64_t begin = uint64_t(R.padded_begin + p);
        const uint64_t w_lo = begin < 2u ? 0u : begin - 2u, w_hi = begin + uint64_t(c.R) + 2u;
        for (int r0 = 0; r0 < R.n_reads; r0 += 64) {
            const int i = r0 + lane;
            bool on = false;
            if (i < R.n_reads)
                on = uint64_t(a.read_begin[R.read_off + i]) < w_hi && w_lo < uint64_t(a.read_end[R.read_off + i]);
            const uint64_t m = __ballot(on);
            if (on) a.keep[keep_off + n_keep + __popcll(m & ((1ull << lane) - 1ull))] = i;
            n_keep += __popcll(m);
        }
    }
    out.n_keep = n_keep;
    if (lane == 0) {
        a.site_out[s] = out;
        GtSite g;
        g.L_off = R.L_off;
        g.al_off = keep_off * kMaxAlleles;
        g.n_haps = nh;
        g.keep_off = int32_t(keep_off);
        g.n_keep = n_keep;
        g.map_off = map_off;
        g.n_alleles = too_many ? 2 : n_alts + 1;   // a skipped site costs one empty sum
        g.out_off = s * kMaxGenotypes;
        a.gt_sites[s] = g;
    }
}

}  // namespace

hipError_t launch_plan_events(const PlanArgs& a, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(a.bitmap, 0, sizeof(uint32_t) * kBitmapWords * size_t(a.n_regions), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gt_plan_events_kernel, dim3(a.n_haps), dim3(64), 0, s, a);
    hipLaunchKernelGGL(gt_plan_scan_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_plan_sites(const PlanArgs& a, int64_t n_sites, hipStream_t s)
{
    if (n_sites <= 0) return hipSuccess;
    hipLaunchKernelGGL(gt_plan_site_kernel, dim3(uint32_t(n_sites)), dim3(64), 0, s, a, int(n_sites));
    return hipGetLastError();
}

}  // namespace hcgt
