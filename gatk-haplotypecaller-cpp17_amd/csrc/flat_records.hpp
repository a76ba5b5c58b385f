// The host record passes of a flat call (flat_plan.cpp), as a host-only body:
// the record format, the packers (scalar and AVX2), and the two passes over the
// caller's pools — scan_pass sizes every record, fold_minis turns the
// per-mini-task sums into offsets, fill_chunk writes records and descriptors
// at those offsets. No HIP call: tests/cpp/flat_records_main.cpp runs the
// passes on exactly sized blocks under ASan / UBSan.
#pragma once
#include <immintrin.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "kernels.hpp"
#include "pool.hpp"
#include "src_view.hpp"

namespace hcphmm {
namespace eng {

constexpr int kMini = 512;              // pairs per mini-task of the host passes

// Per mini-task results of pass 1.
struct Mini {
    int64_t rec = 0, rows = 0, hapw = 0;   // sums, then (after fold_minis) offsets
    int rmax = 0, rmin = INT32_MAX, hmax = 0, hmin = INT32_MAX;
    int nwide = 0;
    bool bad = false;
};

// Gap qualities of a read constant over its rows (blocks of 64 without early
// exit inside a block, so the compiler vectorises the compare).
inline bool constant_gaps_scalar(const uint8_t* i, const uint8_t* d, const uint8_t* c, int len)
{
    const uint8_t i0 = i[0], d0 = d[0], c0 = c[0];
    int k = 0;
    for (; k + 64 <= len; k += 64) {
        uint8_t a = 0;
        for (int j = 0; j < 64; ++j) a |= uint8_t((i[k + j] ^ i0) | (d[k + j] ^ d0) | (c[k + j] ^ c0));
        if (a) return false;
    }
    uint8_t a = 0;
    for (; k < len; ++k) a |= uint8_t((i[k] ^ i0) | (d[k] ^ d0) | (c[k] ^ c0));
    return a == 0;
}

// The same, 32 bytes of each plane per step; the last step overlaps the one
// before instead of a scalar tail.
__attribute__((target("avx2"))) inline __m256i gap_diff32(const uint8_t* i, const uint8_t* d, const uint8_t* c,
                                                           __m256i vi, __m256i vd, __m256i vc)
{
    const __m256i x = _mm256_xor_si256(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(i)), vi);
    const __m256i y = _mm256_xor_si256(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(d)), vd);
    const __m256i z = _mm256_xor_si256(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(c)), vc);
    return _mm256_or_si256(_mm256_or_si256(x, y), z);
}

__attribute__((target("avx2"))) inline bool constant_gaps_avx2(const uint8_t* i, const uint8_t* d, const uint8_t* c,
                                                        int len)
{
    if (len < 32) return constant_gaps_scalar(i, d, c, len);
    const __m256i vi = _mm256_set1_epi8(char(i[0])), vd = _mm256_set1_epi8(char(d[0])),
                  vc = _mm256_set1_epi8(char(c[0]));
    __m256i acc = _mm256_setzero_si256();
    int k = 0;
    for (; k + 32 <= len; k += 32) acc = _mm256_or_si256(acc, gap_diff32(i + k, d + k, c + k, vi, vd, vc));
    if (k < len) {
        const int t = len - 32;
        acc = _mm256_or_si256(acc, gap_diff32(i + t, d + t, c + t, vi, vd, vc));
    }
    return _mm256_testz_si256(acc, acc) != 0;
}

inline bool has_avx2()
{
    static const bool v = __builtin_cpu_supports("avx2");
    return v;
}

constexpr int align4(int x) { return (x + 3) & ~3; }

// Record of a pair (pack_kernels.hip flat_prep_kernel), each field 4-byte
// aligned: the read — one byte per base (kFmtRead1B: quality delta and 2-bit
// code) or its qualities then its code nibbles —, [i, d, c planes], the hap —
// 2-bit codes (kFmtHap2b) or nibbles.
inline int64_t record_bytes(int R, int H, bool planes, int fmt)
{
    return align4(R) + ((fmt & kFmtRead1B) ? 0 : align4((R + 1) / 2)) + (planes ? 3 * int64_t(align4(R)) : 0) +
           ((fmt & kFmtHap2b) ? align4((H + 3) / 4) : align4((H + 1) / 2));
}

// ConvertChar (pairhmm_common.h:26-44): A0 C1 T2 G3 N4, every other byte -> 0.
inline const std::array<uint8_t, 256>& code_table()
{
    static const std::array<uint8_t, 256> t = [] {
        std::array<uint8_t, 256> x{};
        x['C'] = 1;
        x['T'] = 2;
        x['G'] = 3;
        x['N'] = 4;
        return x;
    }();
    return t;
}

// Base codes of n bytes as nibbles, two per byte (byte k/2: code k in the low
// nibble when k is even).
inline void pack_nibbles_scalar(const uint8_t* __restrict s, int n, uint8_t* __restrict d)
{
    const auto& ct = code_table();
    int k = 0;
    for (; k + 1 < n; k += 2) d[k >> 1] = uint8_t(ct[s[k]] | ct[s[k + 1]] << 4);
    if (k < n) d[k >> 1] = ct[s[k]];
}

__attribute__((target("avx2"))) inline __m256i codes32(__m256i v)
{
    // Two nibble lookups instead of four compares: the low nibble gives the
    // code (A 1 -> 0, C 3 -> 1, T 4 -> 2, G 7 -> 3, N E -> 4) and the high
    // nibble that byte must have (4, or 5 for T); any other byte -> 0.
    const __m256i lo = _mm256_and_si256(v, _mm256_set1_epi8(0x0f));
    const __m256i hi = _mm256_and_si256(_mm256_srli_epi16(v, 4), _mm256_set1_epi8(0x0f));
    const __m256i code_lut = _mm256_setr_epi8(0, 0, 0, 1, 2, 0, 0, 3, 0, 0, 0, 0, 0, 0, 4, 0,   //
                                              0, 0, 0, 1, 2, 0, 0, 3, 0, 0, 0, 0, 0, 0, 4, 0);
    const __m256i hi_lut = _mm256_setr_epi8(16, 16, 16, 4, 5, 16, 16, 4, 16, 16, 16, 16, 16, 16, 4, 16,   //
                                            16, 16, 16, 4, 5, 16, 16, 4, 16, 16, 16, 16, 16, 16, 4, 16);
    return _mm256_and_si256(_mm256_cmpeq_epi8(_mm256_shuffle_epi8(hi_lut, lo), hi), _mm256_shuffle_epi8(code_lut, lo));
}

// 32 bytes -> 16 nibble bytes.
__attribute__((target("avx2"))) inline __m128i nibbles32(const uint8_t* s)
{
    const __m256i pairmul = _mm256_set1_epi16(0x1001);   // even byte * 1 + odd byte * 16
    const __m256i p = _mm256_maddubs_epi16(codes32(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(s))), pairmul);
    const __m256i pk = _mm256_permute4x64_epi64(_mm256_packus_epi16(p, p), 0xD8);
    return _mm256_castsi256_si128(pk);
}

__attribute__((target("avx2"))) inline void pack_nibbles_avx2(const uint8_t* __restrict s, int n, uint8_t* __restrict d)
{
    if (n < 32) {
        pack_nibbles_scalar(s, n, d);
        return;
    }
    int k = 0;
    for (; k + 32 <= n; k += 32) _mm_storeu_si128(reinterpret_cast<__m128i*>(d + (k >> 1)), nibbles32(s + k));
    if (k < n) {
        // the last 32 bytes from an even start, overlapping what is written
        // (same values); an odd last byte beyond them alone
        const int t = (n - 32) & ~1;
        _mm_storeu_si128(reinterpret_cast<__m128i*>(d + (t >> 1)), nibbles32(s + t));
        if (t + 32 < n) d[(n - 1) >> 1] = code_table()[s[n - 1]];
    }
}

// Bytes copied 32 at a time, the last 32 overlapping (n >= 32), else memcpy.
__attribute__((target("avx2"))) inline void copy_bytes_avx2(const uint8_t* __restrict s, int n, uint8_t* __restrict d)
{
    if (n < 32) {
        std::memcpy(d, s, size_t(n));
        return;
    }
    int k = 0;
    for (; k + 32 <= n; k += 32)
        _mm256_storeu_si256(reinterpret_cast<__m256i*>(d + k), _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + k)));
    if (k < n)
        _mm256_storeu_si256(reinterpret_cast<__m256i*>(d + n - 32),
                            _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + n - 32)));
}

inline bool constant_gaps(const uint8_t* i, const uint8_t* d, const uint8_t* c, int len)
{
    return has_avx2() ? constant_gaps_avx2(i, d, c, len) : constant_gaps_scalar(i, d, c, len);
}

inline void copy_bytes(const uint8_t* s, int n, uint8_t* d)
{
    if (has_avx2())
        copy_bytes_avx2(s, n, d);
    else
        std::memcpy(d, s, size_t(n));
}

inline void pack_nibbles(const uint8_t* s, int n, uint8_t* d)
{
    if (has_avx2())
        pack_nibbles_avx2(s, n, d);
    else
        pack_nibbles_scalar(s, n, d);
}

// ---- compact record fields (kernels.hpp kFmtRead1B / kFmtHap2b)

// The compact fields, unless HC_PHMM_FLAT_COMPACT=0 (A/B: the nibble records).
inline int compact_fmt()
{
    static const int f = std::getenv("HC_PHMM_FLAT_COMPACT") && std::getenv("HC_PHMM_FLAT_COMPACT")[0] == '0'
                             ? 0
                             : (kFmtRead1B | kFmtHap2b);
    return f;
}

// A read fits one byte per base, ((q & 127) - 33) << 2 | code, when no base
// is 'N' and every quality (& 127) is in [33, 97): SAM's ASCII qualities
// (Phred 0-63 + 33) always are. The quality base is the fixed 33 so the
// check and the packing are one pass (kernels.hpp kFmtRead1B: qbase in the
// descriptor).
constexpr int kQBase = 33;

inline bool read_1b_scalar(const uint8_t* q, const uint8_t* b, int R, uint8_t* d)
{
    const auto& ct = code_table();
    bool ok = true;
    for (int k = 0; k < R; ++k) {
        const int v = (q[k] & 127) - kQBase;
        ok &= unsigned(v) < 64u && b[k] != 'N';
        if (d) d[k] = uint8_t((unsigned(v) << 2) | (ct[b[k]] & 3));   // (unsigned: v < 0 on a read that is refused)
    }
    return ok;
}

// 32 bases: the packed bytes, and the running "bad" accumulator (a delta past
// 63 — qualities below 33 wrap — or an 'N').
__attribute__((target("avx2"))) inline __m256i read_1b32(const uint8_t* q, const uint8_t* b, __m256i& vmax, __m256i& vn)
{
    const __m256i v = _mm256_sub_epi8(
        _mm256_and_si256(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(q)), _mm256_set1_epi8(0x7f)),
        _mm256_set1_epi8(char(kQBase)));
    const __m256i bb = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(b));
    vmax = _mm256_max_epu8(vmax, v);
    vn = _mm256_or_si256(vn, _mm256_cmpeq_epi8(bb, _mm256_set1_epi8('N')));
    // v < 64 where it matters (else the read is refused): the 16-bit shift
    // carries only zero bits across bytes
    return _mm256_or_si256(_mm256_slli_epi16(v, 2), codes32(bb));
}

__attribute__((target("avx2"))) inline bool read_1b_avx2(const uint8_t* q, const uint8_t* b, int R, uint8_t* d)
{
    if (R < 32) return read_1b_scalar(q, b, R, d);
    __m256i vmax = _mm256_setzero_si256(), vn = _mm256_setzero_si256();
    int k = 0;
    for (; k + 32 <= R; k += 32) {
        const __m256i x = read_1b32(q + k, b + k, vmax, vn);
        if (d) _mm256_storeu_si256(reinterpret_cast<__m256i*>(d + k), x);
    }
    if (k < R) {   // the last 32 overlapping what is written (same values)
        const __m256i x = read_1b32(q + R - 32, b + R - 32, vmax, vn);
        if (d) _mm256_storeu_si256(reinterpret_cast<__m256i*>(d + R - 32), x);
    }
    // every delta < 64: no byte of vmax has bit 6 or 7 set
    const __m256i hi = _mm256_and_si256(vmax, _mm256_set1_epi8(char(0xc0)));
    return _mm256_testz_si256(hi, hi) && _mm256_testz_si256(vn, vn);
}

// Pack the read (d may be null: check only); false if it does not fit.
inline bool read_1b(const uint8_t* q, const uint8_t* b, int R, uint8_t* d)
{
    return has_avx2() ? read_1b_avx2(q, b, R, d) : read_1b_scalar(q, b, R, d);
}

// Hap codes 2 bits each (a hap with no 'N'): false if it has one.
inline bool pack_hap_2b_scalar(const uint8_t* s, int n, uint8_t* d)
{
    const auto& ct = code_table();
    bool ok = true;
    for (int k = 0; k < n; k += 4) {
        uint8_t x = 0;
        for (int j = 0; j < 4 && k + j < n; ++j) {
            const uint8_t c = ct[s[k + j]];
            ok &= c != 4;
            x |= uint8_t((c & 3) << (2 * j));
        }
        d[k >> 2] = x;
    }
    return ok;
}

__attribute__((target("avx2"))) inline bool pack_hap_2b_avx2(const uint8_t* s, int n, uint8_t* d)
{
    const __m256i kN = _mm256_set1_epi8('N');
    const __m256i gather = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                            0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
    __m256i vn = _mm256_setzero_si256();
    int k = 0;
    for (; k + 32 <= n; k += 32) {
        const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + k));
        vn = _mm256_or_si256(vn, _mm256_cmpeq_epi8(v, kN));
        // codes c0 + 4 c1 per 16 bits, then (c0 + 4 c1) + 16 (c2 + 4 c3) per 32 bits
        const __m256i t = _mm256_maddubs_epi16(codes32(v), _mm256_set1_epi16(0x0401));
        const __m256i u = _mm256_madd_epi16(t, _mm256_set1_epi32(0x00100001));
        const __m256i g = _mm256_shuffle_epi8(u, gather);
        const uint64_t w = uint64_t(uint32_t(_mm256_extract_epi32(g, 0))) |
                           (uint64_t(uint32_t(_mm256_extract_epi32(g, 4))) << 32);
        std::memcpy(d + (k >> 2), &w, 8);
    }
    const bool ok = k < n ? pack_hap_2b_scalar(s + k, n - k, d + (k >> 2)) : true;
    return ok && _mm256_testz_si256(vn, vn);
}

inline bool pack_hap_2b(const uint8_t* s, int n, uint8_t* d)
{
    return has_avx2() ? pack_hap_2b_avx2(s, n, d) : pack_hap_2b_scalar(s, n, d);
}

inline bool has_n(const uint8_t* s, int n) { return std::memchr(s, 'N', size_t(n)) != nullptr; }

// Why pass 2 refused a part planned without scanning (fill_chunk `retry` bits).
constexpr int kGapsVary = 1;     // a read's gap qualities vary: plan again scanning them (planes)
constexpr int kNotCompact = 2;   // a read or hap does not fit the compact fields: plan again with nibbles

// Pass 2 over mini-tasks [m0, m1): each pair's record at buf + (its offset
// - r0) and its descriptor at dd[k - p0]. With scan_gaps false (pass 1 assumed
// constant gap qualities and format fmt0 everywhere), a read whose gap
// qualities vary sets kGapsVary in `retry` (the part is planned again with
// pass 1 scanning: gapw[k], fmtw[k]); a read that does not fit one byte per
// base, or a hap with an 'N', where fmt0 assumed so, sets kNotCompact (planned
// again with fmt0 = 0, still without scanning).
inline void fill_chunk(const Src& src, int64_t lo, int64_t n, int64_t m0, int64_t m1, const Mini* mini,
                const int32_t* gapw, const uint8_t* fmtw, bool scan_gaps, int fmt0, char* buf, int64_t r0,
                FlatDesc* dd, int64_t p0, std::atomic<int>& retry)
{
    parallel_for(m1 - m0, [&](int64_t a, int64_t e) {
        for (int64_t m = m0 + a; m < m0 + e; ++m) {
            int64_t ro = mini[m].rec, rw = mini[m].rows, hw = mini[m].hapw;
            const int64_t k1 = std::min(n, (m + 1) * kMini);
            for (int64_t k = m * kMini; k < k1; ++k) {
                const int64_t p = lo + k;
                const int R = src.R[p], H = src.H[p];
                const int64_t o = src.read_off[p];
                int32_t g;
                int fmt;
                if (scan_gaps) {
                    g = gapw[k];
                    fmt = fmtw[k];
                } else {
                    const uint8_t *ip = src.ins + o, *dp = src.del + o, *cp = src.gcp + o;
                    if (!constant_gaps(ip, dp, cp, R)) {
                        retry.fetch_or(kGapsVary, std::memory_order_relaxed);
                        return;
                    }
                    g = int32_t((ip[0] & 127) | ((dp[0] & 127) << 7) | ((cp[0] & 127) << 14));
                    fmt = fmt0;
                }
                const int qa = align4(R);
                uint8_t* d = reinterpret_cast<uint8_t*>(buf + (ro - r0));
                size_t at = size_t(qa);
                const int qbase = (fmt & kFmtRead1B) ? kQBase : 0;
                if (fmt & kFmtRead1B) {
                    if (!read_1b(src.q + o, src.rs + o, R, d)) {
                        retry.fetch_or(kNotCompact, std::memory_order_relaxed);   // (scan mode never lists such a read)
                        return;
                    }
                } else {
                    copy_bytes(src.q + o, R, d);
                    pack_nibbles(src.rs + o, R, d + qa);
                    at += size_t(align4((R + 1) / 2));
                }
                if (g < 0) {
                    std::memcpy(d + at, src.ins + o, size_t(R));
                    std::memcpy(d + at + qa, src.del + o, size_t(R));
                    std::memcpy(d + at + 2 * qa, src.gcp + o, size_t(R));
                    at += 3 * size_t(qa);
                }
                if (fmt & kFmtHap2b) {
                    if (!pack_hap_2b(src.hap + src.hap_off[p], H, d + at)) {
                        retry.fetch_or(kNotCompact, std::memory_order_relaxed);
                        return;
                    }
                } else {
                    pack_nibbles(src.hap + src.hap_off[p], H, d + at);
                }
                dd[k - p0] = FlatDesc{ro, int(rw), R, H, int(hw), g, fmt | (qbase << 8)};
                ro += record_bytes(R, H, g < 0, fmt);
                rw += qa;
                hw += hap_table_words(H);
            }
        }
    }, 1);
}

// Pass 1 over pairs [lo, lo + n): per mini-task sums and bounds; with
// scan_gaps, each read's constant gap triple (or -1) in gapw and its format
// (compact fields where they fit, if compact_fmt() allows) in fmtw; without,
// every pair is assumed to take format fmt0; every stride-th hap length in hsamp.
inline void scan_pass(const Src& src, int64_t lo, int64_t n, bool scan_gaps, int fmt0, Mini* mini, int32_t* gapw,
               uint8_t* fmtw, int32_t* hsamp, int64_t stride)
{
    const int64_t nmini = (n + kMini - 1) / kMini;
    parallel_for(nmini, [&](int64_t m0, int64_t m1) {
        for (int64_t m = m0; m < m1; ++m) {
            Mini& M = mini[m];
            const int64_t a = m * kMini, e = std::min(n, a + kMini);
            for (int64_t k = a; k < e; ++k) {
                const int64_t p = lo + k;
                const int R = src.R[p], H = src.H[p];
                if (R <= 0 || R > HC_PHMM_MAX_READ_LEN || H <= 0 || H > HC_PHMM_MAX_HAP_LEN) {
                    M.bad = true;
                    gapw[k] = 0;
                    continue;
                }
                int32_t g = 0;
                int fmt = fmt0;   // assumed (checked by pass 2) unless scanning
                if (scan_gaps) {
                    const int64_t o = src.read_off[p];
                    const uint8_t *ip = src.ins + o, *dp = src.del + o, *cp = src.gcp + o;
                    g = constant_gaps(ip, dp, cp, R)
                            ? int32_t((ip[0] & 127) | ((dp[0] & 127) << 7) | ((cp[0] & 127) << 14))
                            : -1;
                    gapw[k] = g;
                    fmt = compact_fmt() == 0 ? 0
                                             : (read_1b(src.q + o, src.rs + o, R, nullptr) ? kFmtRead1B : 0) |
                                                   (has_n(src.hap + src.hap_off[p], H) ? 0 : kFmtHap2b);
                    fmtw[k] = uint8_t(fmt);
                }
                M.rec += record_bytes(R, H, g < 0, fmt);
                M.rows += align4(R);
                M.hapw += hap_table_words(H);
                M.rmax = std::max(M.rmax, R);
                M.rmin = std::min(M.rmin, R);
                M.hmax = std::max(M.hmax, H);
                M.hmin = std::min(M.hmin, H);
                M.nwide += H > kSeg64MaxH;
                if (k % stride == 0) hsamp[k / stride] = H;
            }
        }
    }, 8);
}

// A part's bounds and totals over its mini-tasks (pass 1's sums).
struct FlatTotals {
    int rmax = 0, rmin = INT32_MAX, hmax = 0, hmin = INT32_MAX;
    int64_t nwide = 0, rec = 0, rows = 0, hapw = 0;
    bool bad = false;   // a pair with an invalid read or hap length
};

// The fold between the passes: each mini-task's sums become its offsets
// (exclusive running sums, as fill_chunk reads them); returns the totals.
inline FlatTotals fold_minis(Mini* mini, int64_t nmini)
{
    FlatTotals t;
    for (int64_t m = 0; m < nmini; ++m) {
        Mini& M = mini[m];
        t.bad |= M.bad;
        t.rmax = std::max(t.rmax, M.rmax);
        t.rmin = std::min(t.rmin, M.rmin);
        t.hmax = std::max(t.hmax, M.hmax);
        t.hmin = std::min(t.hmin, M.hmin);
        t.nwide += M.nwide;
        const int64_t r = M.rec, w = M.rows, h = M.hapw;
        M.rec = t.rec;
        M.rows = t.rows;
        M.hapw = t.hapw;
        t.rec += r;
        t.rows += w;
        t.hapw += h;
    }
    return t;
}

// Does a sample of the part's pairs (every stride-th, at most ~1 024) all fit
// the compact fields? Real reads often hold an 'N': such a part then starts
// with the nibble fields instead of finding out in pass 2, where the refusal
// costs the chunks filled so far and a second planning (advisor round 5).
inline bool sample_fits_compact(const Src& src, int64_t lo, int64_t n)
{
    if (compact_fmt() == 0) return false;
    const int64_t stride = std::max<int64_t>(1, n / 1024);
    for (int64_t k = 0; k < n; k += stride) {
        const int64_t p = lo + k, o = src.read_off[p];
        const int R = src.R[p], H = src.H[p];
        if (R <= 0 || H <= 0) continue;   // (pass 1 refuses the part)
        if (!read_1b(src.q + o, src.rs + o, R, nullptr) || has_n(src.hap + src.hap_off[p], H)) return false;
    }
    return true;
}

}  // namespace eng
}  // namespace hcphmm
