// Device building blocks shared by the column-segmented PairHMM kernels
// (lane_kernel.hip: phmm_seg_kernel, phmm_seg64_kernel, the one-lane kernel):
// the cell update in the reference's operation order, the per-row constants,
// DPP hand-offs, prefetch depth.
// Same semantics as compute_full_prob_avx{s,d} (avx-pairhmm-template.h:210-346).
#pragma once
#include <type_traits>

#include "device_common.hpp"
#include "kernels.hpp"
#include "luts.hpp"
#include "seg_spread.hpp"

namespace hcphmm {
namespace seg {

template <typename T> __device__ __forceinline__ T initial_value();
template <> __device__ __forceinline__ float initial_value<float>() { return 0x1p120f; }    // Context.h:149
template <> __device__ __forceinline__ double initial_value<double>() { return 0x1p1020; }  // Context.h:109

template <typename T>
struct RowConst {
    T pm, px;        // prior: 1 - ph2pr[q], ph2pr[q] / 3          (this row)
    T my, yy;        // Y transitions: ph2pr[d], ph2pr[c]           (this row)
    T mm, g, mx, xx; // transitions into the NEXT row: mm, 1 - ph2pr[c], ph2pr[i], ph2pr[c]
    int rc;          // read base code of this row
};

// initializeVectors / stripeINITIALIZATION (avx-pairhmm-template.h:83-177):
// wc = this row's packed word, wn = the next row's.
template <typename T>
__device__ __forceinline__ void row_const(const T* __restrict__ lut, uint32_t wc, uint32_t wn, RowConst<T>& k)
{
    const T* __restrict__ ph2pr = lut + kOffPh2pr;
    k.pm = lut[kOffPm + row_q(wc)];
    k.px = lut[kOffPx + row_q(wc)];
    k.my = ph2pr[row_d(wc)];
    k.yy = ph2pr[row_c(wc)];
    k.mm = lut[kOffMM + mm_idx(row_i(wn), row_d(wn))];
    k.g = lut[kOffGapm + row_c(wn)];
    k.mx = ph2pr[row_i(wn)];
    k.xx = ph2pr[row_c(wn)];
    k.rc = row_rc(wc);
}

// Prior of the next column of a match word. The window is MSB-first and a row
// consumes it strictly left to right, so one add with carry-out (w + w:
// v_add_co_u32, half rate) both shifts the window one column left and puts the
// column's bit into VCC for every lane; a VCC-form v_cndmask_b32 (e32, full
// rate; two for a double) then picks pm or px: 3 issue slots per fp32 cell
// where v_bfe_i32 + v_bitop3_b32 took 4, and no register besides the window
// word, which is dead after the row anyway. Plain C, so the compiler itself
// keeps the VCC write and its read the required wait states apart. The word is
// consumed: the caller reloads it before its next row.
template <typename T>
__device__ __forceinline__ T prior_next(uint32_t& w, T pm, T px)
{
    const bool c = __builtin_uadd_overflow(w, w, &w);
    return c ? pm : px;
}

// Column J of one row of one block; recursion unrolls the row at compile time.
// M enters as M[i][c0+J+1] (= T_old[J-1] * prior). Before T[J] is overwritten,
// its old value (the next column's diagonal) is consumed into the next M, so
// the new T[J] can take the old one's register: no copies between rows.
// mw0/mw1: the row's match words for block columns 1-32 / 33-64, consumed
// MSB-first in column order by prior_next (the caller took column 1's bit of
// mw0 for M; column J+1 shifts word (J+1) >> 5).
// EQ: mx == my bitwise (insertion and deletion gap qualities equal on every
// row: the reference's SAMRecord passes 'I' for both, sam.hpp:30-32), so the
// product M*mx that feeds X[J] is also the M*my term of the next column's Y:
// one multiply fewer per cell, the same rounded values. Ml then carries that
// product instead of M.
// MASK (the one-lane kernel, whose blocks start at column 1): only columns
// J < lim enter the sums (lim = columns of the block inside the hap on the
// pair's last row, else 0).
template <typename T, int BC, int J, int NC, bool SUM, bool EQ, bool MASK = false>
__device__ __forceinline__ void cell(T (&Tt)[BC], T (&X)[BC], T M, T& Ml, T& Yl, uint32_t& mw0, uint32_t& mw1,
                                     T pm, T px, const RowConst<T>& k, int lim, T& sumM, T& sumX)
{
    if constexpr (J < NC) {
        // AHEAD: the shift of column J+1 is issued ahead of two independent
        // multiplies and its select after them (scheduling barriers), so the
        // carry's way through VCC is covered inside the wave. That pays where
        // a wave runs alone on its SIMD (fp64 rescues, the narrow blocks of
        // small batches); wide fp32 blocks, which run three waves per SIMD,
        // are faster in the compiler's own order.
        constexpr bool AHEAD = !MASK && (sizeof(T) == 8 || BC <= 32);
        T Mn = M;
        if constexpr (!AHEAD && J + 1 < NC)
            Mn = Tt[J] * prior_next(((J + 1) >> 5) ? mw1 : mw0, pm, px);
        const T Xc = X[J];
        T Mm = T(0), Xg = T(0);
        if constexpr (AHEAD) {
            bool cb = false;
            if constexpr (J + 1 < NC) {
                uint32_t& w = ((J + 1) >> 5) ? mw1 : mw0;
                cb = __builtin_uadd_overflow(w, w, &w);
                __builtin_amdgcn_sched_barrier(0);
            }
            Mm = M * k.mm;
            Xg = Xc * k.g;
            if constexpr (J + 1 < NC) {
                __builtin_amdgcn_sched_barrier(0);
                Mn = Tt[J] * (cb ? pm : px);
            }
        }
        if constexpr (SUM && !MASK) {
            // The row sums first: they read M and the old X[J] before X[J] is
            // rewritten (after it, the old value needed a copy per column).
            // Every column of a block is a hap column or a zero padding column
            // (run_seg), so the row's sums need no column mask; rows other than
            // the pair's last accumulate values that run_seg discards.
            sumM = sumM + M;
            sumX = sumX + Xc;
        }
        T Y;
        if constexpr (EQ) {
            const T Mx = M * k.mx;
            Y = (J == 0) ? Yl : (Ml + Yl * k.yy);
            if constexpr (AHEAD)
                Tt[J] = (Mm + Xg) + Y * k.g;
            else
                Tt[J] = (M * k.mm + Xc * k.g) + Y * k.g;
            X[J] = Mx + Xc * k.xx;
            Ml = Mx;
        } else {
            Y = (J == 0) ? Yl : (Ml * k.my + Yl * k.yy);
            if constexpr (AHEAD)
                Tt[J] = (Mm + Xg) + Y * k.g;
            else
                Tt[J] = (M * k.mm + Xc * k.g) + Y * k.g;
            X[J] = M * k.mx + Xc * k.xx;
            Ml = M;
        }
        if constexpr (SUM && MASK) {
            const bool c = J < lim;   // column c0+J+1 <= H on the pair's last row
            sumM = sumM + (c ? M : T(0));
            sumX = sumX + (c ? Xc : T(0));
        }
        Yl = Y;
        cell<T, BC, J + 1, NC, SUM, EQ, MASK>(Tt, X, Mn, Ml, Yl, mw0, mw1, pm, px, k, lim, sumM, sumX);
    }
}

// Y entering the column after the last one of a row segment: Ml*my + Yl*yy
// (EQ: Ml already holds M*mx = M*my).
template <bool EQ, typename T>
__device__ __forceinline__ T y_next(T Ml, T Yl, T my, T yy)
{
    if constexpr (EQ)
        return Ml + Yl * yy;
    else
        return Ml * my + Yl * yy;
}

// The fp32 constant-gap path takes its priors from LDS instead of selecting
// them: two adjacent columns of a row take one of four (prior, prior) pairs that
// depend only on the row's quality q and the two columns' match bits, so each
// workgroup of seg waves keeps ptab[128][4] of float2 (4 KB, fill_shared_tabs),
//   ptab[q][p] = { p & 2 ? pm[q] : px[q],  p & 1 ? pm[q] : px[q] }
// (the pair's first column is the higher bit, as in the MSB-first window), and a
// row reads one ds_read_b64 per two columns. The address is the row's table
// base (32-byte aligned, once per row) with the two window bits placed at bits
// 4:3 — a shift (1 slot) and a v_and_or_b32 (a three-source form, 2 slots): 3
// VALU slots per two columns where the carry select (prior_next) takes 6, and
// the reads issue on the LDS port beside the other waves' VALU work. The floats
// multiplied are the ones the select picks, so the results are the same bits.
constexpr int kPtabPairs = kQuals * 4 * 2;    // floats of the pair table
constexpr int kPtabLen = kPtabPairs + 2 * kQuals;   // then pm[128], px[128] for the rows that keep the select

typedef float float2v __attribute__((ext_vector_type(2)));
using lds_cfloat2 = const __attribute__((address_space(3))) float2v;
// LDS byte address of a pointer into a __shared__ array.
__device__ __forceinline__ uint32_t lds_addr(const void* p)
{
    return uint32_t(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) void*)p));
}

// Table base of a row: ptab's LDS address + 32 * q.
__device__ __forceinline__ uint32_t ptab_row(uint32_t ptab_lds, uint32_t w) { return ptab_lds + (row_q(w) << 5); }

// The priors of block columns 2p, 2p+1 (0-based) of a row with table base
// `base` and match words m (MSB first: column c is bit 31 - (c & 31) of word c >> 5).
template <int P>
__device__ __forceinline__ float2 ptab_pair(uint32_t base, const uint2& m)
{
    constexpr int sh = 30 - 2 * (P & 15);
    const uint32_t w = (P >> 4) ? m.y : m.x;
    uint32_t bits;
    if constexpr (sh >= 3)
        bits = w >> (sh - 3);
    else
        bits = w << (3 - sh);
    const float2v v = *reinterpret_cast<lds_cfloat2*>(base | (bits & 24u));
    return make_float2(v.x, v.y);
}

// pm[q] and px[q] alone, for the rows that keep the select: the arrays behind
// the pair table (fp32; read from the table's own rows, 32 bytes apart, the
// lanes of a wave meet on 8 banks) or the prior tables (fp64, load_slut).
__device__ __forceinline__ float lds_pm(const float* __restrict__ ptab, int q) { return ptab[kPtabPairs + q]; }
__device__ __forceinline__ float lds_px(const float* __restrict__ ptab, int q) { return ptab[kPtabPairs + kQuals + q]; }
__device__ __forceinline__ double lds_pm(const double* __restrict__ slut, int q) { return slut[kOffPm + q]; }
__device__ __forceinline__ double lds_px(const double* __restrict__ slut, int q) { return slut[kOffPx + q]; }

// Block widths that take their priors from the table. Blocks of at most 32
// columns are what small batches run, one round of waves at one or two per
// SIMD: there the step is short, the two dependent LDS reads between rows
// (window, then first pair) are not covered, and the select with its shift
// issued ahead (cell, AHEAD) is faster (S1 at 14 columns 0.0560 -> 0.0580 ms
// with the table, S4 at 24-32 0.671 -> 0.694; profiles/r10_prior_table_ab.jsonl).
constexpr int kPtabMinWidth = 34;

// Pairs a row holds: the one its cells consume and the one in flight, read
// three columns ahead of its first use. One pair (read one column ahead)
// leaves the wave waiting on the LDS, three measure no better than two (S2 fp32
// pass 7.85 / 7.75 / 7.74 ms, profiles/r10_prior_table_ab.jsonl): by then the
// LDS array itself is the limit.
constexpr int kPtabAhead = 2;

// The quad table: the same priors indexed by FOUR match bits, so one address
// and one 16-byte read (ds_read_b128) serve four columns, where the pair table
// takes a shift, a v_and_or_b32 and a ds_read_b64 per two. A quality row holds
// 16 patterns of float4, 256 bytes:
//   tab[r][c] = priors of the group's columns 0, 1, 2, 3 (pattern bits 3 .. 0
//               choose pm or px; the group's first column is the highest bit,
//               as in the MSB-first window).
// A row covers all 64 banks, so the row does not pick the banks, only the
// 16-byte column slot does, and the skewed pattern distribution (match bits
// at p = 0.25) piles the 16 lanes of a ds_read_b128 service group onto a few
// slots. The physical column is c = pattern ^ (q & 15), which spreads lanes on
// different rows over all 16 slots (tools/lds_quad_model.py: 19.9 LDS cycles
// per four columns without, 11.6 with; two ds_read_b64 of 128-byte rows took
// 12.5).
// The table is the workgroup's, kQuadRows = 64 rows indexed by the absolute
// quality, filled once by all its waves (fill_shared_tabs): the row of quality
// byte q is q & 63 and the table holds the bytes kQuadQ0 = 33 .. 96, Phred 0 ..
// 63 of a SAM quality string. A wave takes it when every quality of its reads
// is one of those (quad_scan); the others keep the pair table, the
// workgroup's too. What a wave keeps for
// itself is its match window, and a quad wave keeps it SPREAD (seg_spread.hpp):
// one byte per group of four columns holding pattern << 4, so a group's table
// address is base2 ^ byte, one ds_read_u8 (no VALU slot) and one v_xor_b32,
// where the packed window took a shift and a v_and_or_b32 (3 slots). base2 is
// the row's base with its swizzle nibble already at bits 7:4 (a row is
// 256-byte aligned, so (base | n << 4) ^ (p << 4) == base | ((p ^ n) << 4)):
// no per-row XOR of the window and no replicated nibble.
// HC_PTAB_NO_QUAD (EXTRA_DEV_FLAGS, A/B builds): every width keeps the pair
// table and the packed window; the byte form is compiled out.
// HC_QUAD_NO_SWIZZLE (likewise): the physical column is the pattern.
#ifdef HC_QUAD_NO_SWIZZLE
constexpr bool kQuadSwizzle = false;
#else
constexpr bool kQuadSwizzle = true;
#endif
constexpr int kQuadRows = 64;
constexpr int kQuadQ0 = 33;   // the lowest quality byte the table holds (Phred 0)
constexpr int kQuadRowBytes = 256;
// Widths whose quad form fits the register budget (168 VGPRs, no scratch).
#ifdef HC_PTAB_NO_QUAD
constexpr int kQuadMinWidth = 1 << 30, kQuadMaxWidth = 0;
constexpr int kQuadLen = 0;
constexpr int kWindowBytes = 5 * 64 * 8;
#else
constexpr int kQuadMinWidth = kPtabMinWidth, kQuadMaxWidth = 64;
constexpr int kQuadLen = kQuadRows * kQuadRowBytes / 4;   // floats of the quad table
constexpr int kWindowBytes = kSpreadWaveBytes;            // a wave's window, packed (2 560) or spread
#endif
template <typename T, int BC>
constexpr bool quad_width()
{
    return std::is_same<T, float>::value && BC >= kQuadMinWidth && BC <= kQuadMaxWidth;
}

// Wave-uniform max / min of a per-lane int (once per wave).
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return __builtin_amdgcn_readfirstlane(v);
}

// The workgroup's tables, filled by all its nt threads (thread t): the pair
// table with its pm / px arrays (two 16-byte stores per quality) and the quad
// table (one 16-byte store per row and pattern). The caller's __syncthreads()
// follows.
__device__ __forceinline__ void fill_ptab(float* __restrict__ ptab, const float* __restrict__ lut, int t, int nt)
{
    for (int q = t; q < kQuals; q += nt) {
        const float pm = lut[kOffPm + q], px = lut[kOffPx + q];
        float4* d = reinterpret_cast<float4*>(ptab + q * 8);
        d[0] = make_float4(px, px, px, pm);   // patterns 00, 01
        d[1] = make_float4(pm, px, pm, pm);   // patterns 10, 11
        ptab[kPtabPairs + q] = pm;
        ptab[kPtabPairs + kQuals + q] = px;
    }
}
__device__ __forceinline__ void fill_qtab(float* __restrict__ qtab, const float* __restrict__ lut, int t, int nt)
{
    for (int e = t; e < kQuadLen / 4; e += nt) {
        const int r = e >> 4, p = e & 15;
        const int q = kQuadQ0 + ((r - kQuadQ0) & (kQuadRows - 1));   // the byte of the table's range with q & 63 == r
        const float pm = lut[kOffPm + q], px = lut[kOffPx + q];
        const int c = kQuadSwizzle ? p ^ (r & 15) : p;
        *reinterpret_cast<float4*>(qtab + r * (kQuadRowBytes / 4) + c * 4) =
            make_float4((p & 8) ? pm : px, (p & 4) ? pm : px, (p & 2) ? pm : px, (p & 1) ? pm : px);
    }
}
__device__ __forceinline__ void fill_shared_tabs(float* __restrict__ ptab, float* __restrict__ qtab,
                                                 const float* __restrict__ lut, int t, int nt)
{
    fill_ptab(ptab, lut, t, nt);
    fill_qtab(qtab, lut, t, nt);
}

// base2 of a read row with quality byte q: the table row q & 63 (a prefetched row
// outside every read can carry any quality; the mask keeps its address inside
// the table and no result depends on what it selects) with the swizzle nibble
// q & 15 at bits 7:4.
__device__ __forceinline__ uint32_t quad_base2(uint32_t qtab_lds, uint32_t w)
{
    return qtab_lds + (((w & 63u) << 8) | (kQuadSwizzle ? (w & 15u) << 4 : 0u));
}

// A row's table base from its row word (QUAD: base2 of the quad table).
template <bool QUAD>
__device__ __forceinline__ uint32_t tab_row(uint32_t tab_lds, uint32_t w)
{
    if constexpr (QUAD)
        return quad_base2(tab_lds, w);
    else
        return ptab_row(tab_lds, w);
}

// The byte of column group G (block columns 4G .. 4G+3) of the lane's spread
// window: slot is the LDS address of the row's (read code, lane). The last
// group of a width that is no multiple of 4 takes its low two bits from the
// window's next columns; an entry's .x and .y do not depend on them.
using lds_cbyte = const __attribute__((address_space(3))) uint8_t;
template <int G>
__device__ __forceinline__ uint32_t win_byte(uint32_t slot)
{
    return *reinterpret_cast<lds_cbyte*>(slot + spread_group_off(G));
}
// The priors of a group from its byte: the pattern at bits 7:4 meets the row's
// swizzle nibble there.
typedef float float4v __attribute__((ext_vector_type(4)));
using lds_cfloat4 = const __attribute__((address_space(3))) float4v;
__device__ __forceinline__ float4 quad_read(uint32_t base2, uint32_t byte)
{
    const float4v v = *reinterpret_cast<lds_cfloat4*>(base2 ^ byte);
    return make_float4(v.x, v.y, v.z, v.w);
}

// What one table read gives and a row keeps a ring of: entry E of a row is a
// pair of columns' priors (pair table) or a group of four (quad table).
template <bool QUAD> using TabEnt = std::conditional_t<QUAD, float4, float2>;
__device__ __forceinline__ float ent_el(const float2& v, int e) { return e ? v.y : v.x; }
__device__ __forceinline__ float ent_el(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// What a table row reads its entries with. Pair table: the row's base and its
// packed window. Quad table: base2, the lane's window slot and the byte of the
// next group to read, requested one group before its address is formed.
template <bool QUAD> struct TabRow;
template <> struct TabRow<false> {
    uint32_t base;
    uint2 m;
};
template <> struct TabRow<true> {
    uint32_t base, slot, byte;
};

// Column J of one row, fp32 EQ path with table priors: `cell`'s EQ arithmetic
// in the same order. An entry holds the priors of N columns (pair table 2,
// quad table 4) and pr is a ring of D = 2 entries: on entry to column J = N e
// it holds entries e and e + 1. The column N e + N - 2 takes its successor's
// prior, entry e's last element and last use, and then issues the read of
// entry e + 2 into entry e's registers, 2N - 1 columns ahead of its first use
// (pairs 3, groups 5). The first scheduling barrier keeps that multiply ahead
// of the read (behind it, the read needs registers of its own), the second
// lets VALU work through and keeps the LDS reads where they are (hoisted to
// the row's start they take an entry's registers each, sunk to their use the
// wave waits on every one).
// QUAD: with the read of group e + 2 goes the request of group e + 3's byte,
// so a byte is in flight for a whole group before its address is formed. A
// width with BC % 4 == 2 ends in a half group: its read takes 16 bytes and the
// cells use .x and .y.
template <int BC, int J, bool SUM, int D, bool QUAD>
__device__ __forceinline__ void cell_tab(float (&Tt)[BC], float (&X)[BC], float M, float& Ml, float& Yl,
                                         TabEnt<QUAD> (&pr)[D], TabRow<QUAD>& tr, const RowConst<float>& k,
                                         float& sumM, float& sumX)
{
    constexpr int N = QUAD ? 4 : 2;           // columns per entry
    constexpr int NE = (BC + N - 1) / N;      // entries of a row
    if constexpr (J < BC) {
        float Mn = M;
        if constexpr (J + 1 < BC) Mn = Tt[J] * ent_el(pr[((J + 1) / N) % D], (J + 1) % N);
        if constexpr (J % N == N - 2 && J / N + D < NE) {
            constexpr int kNoDs = 0x2 | 0x4 | 0x10 | 0x20 | 0x40;   // VALU, SALU and VMEM may cross; DS may not
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (QUAD) {
                pr[(J / N + D) % D] = quad_read(tr.base, tr.byte);
                if constexpr (J / N + D + 1 < NE) tr.byte = win_byte<J / N + D + 1>(tr.slot);
            } else {
                pr[(J / N + D) % D] = ptab_pair<J / N + D>(tr.base, tr.m);
            }
            __builtin_amdgcn_sched_barrier(kNoDs);
        }
        const float Xc = X[J];
        if constexpr (SUM) {
            sumM = sumM + M;
            sumX = sumX + Xc;
        }
        const float Mx = M * k.mx;
        const float Y = (J == 0) ? Yl : (Ml + Yl * k.yy);
        Tt[J] = (M * k.mm + Xc * k.g) + Y * k.g;
        X[J] = Mx + Xc * k.xx;
        Ml = Mx;
        Yl = Y;
        cell_tab<BC, J + 1, SUM, D, QUAD>(Tt, X, Mn, Ml, Yl, pr, tr, k, sumM, sumX);
    }
}

// A lane's pair: its read rows and hap match table as 32-bit offsets from the
// part's uniform bases (one VGPR each per lane and SGPR bases, so the loads
// take the global_load SGPR-base + VGPR-offset form and no 64-bit address
// stays live per lane: they spilled).
struct LaneCtx {
    const uint32_t* rbase;  // rows - kRowPadBefore (uniform)
    uint32_t rbyte;         // byte offset of the read's first row word from rbase
    const uint32_t* hbase;  // the part's hap tables (uniform)
    uint32_t hbyte;         // byte offset of the hap's match table from hbase
    int R, H;
};

// Row word idx of the lane's read (idx may be negative, down to
// -kRowPadBefore: prefetches before a read's first row).
__device__ __forceinline__ uint32_t row_word(const LaneCtx& cx, int idx)
{
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(cx.rbase) +
                                             (cx.rbyte + unsigned(idx) * 4u));
}
// Word idx of the lane's hap match table.
__device__ __forceinline__ uint32_t hap_word(const LaneCtx& cx, int idx)
{
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(cx.hbase) +
                                             (cx.hbyte + unsigned(idx) * 4u));
}

// Row-0 diagonal T0 = (0*mm + 0*gapm) + (INITIAL/H)*gapm with row 1's
// constants (avx-pairhmm-template.h:160-166: Y[0][j] = INITIAL / H).
template <typename T>
__device__ __forceinline__ T row0_t(const T* __restrict__ lut, uint32_t w1, int H)
{
    const T mm1 = lut[kOffMM + mm_idx(row_i(w1), row_d(w1))];
    // Opaque offset: otherwise the address lut + 4 * row_c is shared with row
    // 1's ph2pr[row_c] load in the step loop's set-up, and that 64-bit address,
    // live across the wave's whole prologue, is spilled to scratch.
    unsigned go = unsigned(kOffGapm + row_c(w1)) * unsigned(sizeof(T));
    asm volatile("" : "+v"(go));
    const T g1 = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(lut) + go);
    const T initY = initial_value<T>() / T(H);
    return (T(0) * mm1 + T(0) * g1) + initY * g1;
}

__device__ __forceinline__ LaneCtx desc_ctx(const PairDesc pd, const uint32_t* rows, const uint32_t* hapw)
{
    return LaneCtx{rows - kRowPadBefore, unsigned(pd.x + kRowPadBefore) * 4u, hapw, unsigned(pd.z) * 4u, pd.y, pd.w};
}
__device__ __forceinline__ LaneCtx pair_ctx(const PairDesc* pairs, const uint32_t* rows, const uint32_t* hapw,
                                            int pid)
{
    return desc_ctx(pairs[pid], rows, hapw);
}

// Constant-gap tag of a read: bit 31 of its first row word (pack_reads_kernel).
// EQ additionally needs insertion == deletion gap quality.
__device__ __forceinline__ bool read_cg(uint32_t w1) { return (w1 >> 31) != 0; }
__device__ __forceinline__ bool read_eq(uint32_t w1) { return read_cg(w1) && row_i(w1) == row_d(w1); }

__device__ __forceinline__ float from_left(float v)
{
    // DPP wave_shr:1: lane l receives lane l-1's v; lane 0 receives 0 by
    // bound_ctrl (no zeroed destination to materialise first).
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ double from_left(double v)
{
    const long long x = __double_as_longlong(v);
    const unsigned lo = unsigned(__builtin_amdgcn_mov_dpp(int(x), 0x138, 0xf, 0xf, true));
    const unsigned hi = unsigned(__builtin_amdgcn_mov_dpp(int(x >> 32), 0x138, 0xf, 0xf, true));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// v & mask bitwise (mask all ones or zero, in a VGPR): one full-rate v_and per
// 32 bits. (Written as C the compiler proves the mask boolean and selects with
// v_cndmask on an SGPR lane mask instead, a half-rate form.)
__device__ __forceinline__ uint32_t and_v(uint32_t a, uint32_t m)
{
    uint32_t r;
    asm("v_and_b32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(m));
    return r;
}
// AND: the v_and form (the mask lives in a VGPR: one register more, so only
// where the block's registers leave room — the widest fp32 blocks spill with it).
template <bool AND>
__device__ __forceinline__ float masked(float v, uint32_t m)
{
    return __uint_as_float(AND ? and_v(__float_as_uint(v), m) : (__float_as_uint(v) & m));
}
template <bool AND>
__device__ __forceinline__ double masked(double v, uint32_t m)
{
    const unsigned long long x = (unsigned long long)__double_as_longlong(v);
    if (!AND) return __longlong_as_double((long long)(x & ((unsigned long long)m << 32 | m)));
    return __longlong_as_double(
        (long long)(((unsigned long long)and_v(uint32_t(x >> 32), m) << 32) | and_v(uint32_t(x), m)));
}


// Step bounds of a column-segmented wave (wave-uniform).
struct SegSteps {
    int rmax;     // max R of the wave's pairs
    int rmin;     // first step that may need the row sums
    int nsteps;   // max over the wave's pairs of R + nb - 1
    int prio = 0; // issue priority: 0 off, 1 by remaining steps, 2 by age (set_prio)
    unsigned long long t0 = 0;   // the wave's start (s_memrealtime), for prio 2
};

// VALU issue between the waves of a SIMD is arbitrated by priority, then age
// (MI355X_MICROARCH.md, two waves per SIMD): the oldest wave runs ahead and
// the last waves of a pass, the youngest, are left to finish alone at half
// the issue rate. With prio on, a wave raises its priority with the steps it
// has left (longest remaining first), so co-resident waves tend to finish
// together. s_setprio takes an immediate: four uniform branches.
__device__ __forceinline__ void set_prio_by_remaining(int rem)
{
    if (rem > 192) __builtin_amdgcn_s_setprio(3);
    else if (rem > 96) __builtin_amdgcn_s_setprio(2);
    else if (rem > 32) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}
// In a pass whose waves are fetched from a counter, a hardware wave keeps its
// slot for the whole launch, so between the two waves of a SIMD the older
// always wins a tie: with chains of four, one wave per SIMD took 3.2 ms while
// the other slot ran four 0.78 ms chains (tools/chain_probe.py, DESIGN.md
// §16.2), and neither the remaining-steps bands nor bands by progress undid
// it (a fresh wave on the older slot ties or outranks the starved one). There
// the priority rises with the time since the wave's start instead (quanta of
// ~100 us): the wave that started first goes first, as if each wave were a
// fresh hardware wave dispatched in order.
__device__ __forceinline__ void set_prio_by_age(unsigned long long t0)
{
    const unsigned long long q = (__builtin_amdgcn_s_memrealtime() - t0) / 10000;   // 100 MHz ticks
    if (q >= 3) __builtin_amdgcn_s_setprio(3);
    else if (q == 2) __builtin_amdgcn_s_setprio(2);
    else if (q == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}
// prio mode: 1 by remaining steps, 2 by the wave's age (SegSteps::prio).
__device__ __forceinline__ void set_prio(int mode, int kk, int nsteps, unsigned long long t0)
{
    if (mode == 2) set_prio_by_age(t0);
    else set_prio_by_remaining(nsteps - kk);
}

// Rows of read words a lane keeps in flight (loaded PD steps before use). A
// lone step of a narrow block is too short to cover a global load, so narrow
// blocks prefetch deeper; the step loop is unrolled by PD so every word lands
// in its own register and is not touched (no wait) until its step. fp32
// blocks of 32-64 columns take two steps too (round 3: S2 fp32 pass 8.884 ->
// 8.815 ms, a 125k-pair shard -1.5 %, S1w at 1M pairs +0.8 %; three steps no
// better: profiles/r03_prefetch_depth_ab.jsonl).
template <typename T, int BC>
constexpr int seg_prefetch()
{
    return sizeof(T) == 8 ? (BC >= 16 ? 1 : 2) : (BC >= 16 ? 2 : 4);
}

// Call f(integral_constant<P>) for P = 0 .. N-1 (compile-time phases).
template <int P, int N, typename F>
__device__ __forceinline__ void for_phases(F&& f)
{
    if constexpr (P < N) {
        f(std::integral_constant<int, P>{});
        for_phases<P + 1, N>(f);
    }
}

// The prior tables [ph2pr | pm | px | gapm] (luts.hpp) in LDS: the per-row
// prior lookups of the segmented kernels read them there.
constexpr int kSlutLen = kOffMM;
template <typename T>
__device__ __forceinline__ void load_slut(T* __restrict__ slut, const T* __restrict__ lut)
{
    for (int t = threadIdx.x; t < kSlutLen; t += blockDim.x) slut[t] = lut[t];
    __syncthreads();
}

// Block widths of fp32 column-segmented waves (LaneWave.ncols of a seg wave):
// 8..64 in steps of 2 (steps of 4 measured the same kernel time at a worse
// column rounding; odd widths model only 0.6 % better).
#define HC_SEG_WIDTHS(X)                                                                                       \
    X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28) X(30) X(32) X(34) X(36) X(38) X(40) X(42) \
    X(44) X(46) X(48) X(50) X(52) X(54) X(56) X(58) X(60) X(62) X(64)

// A pair's nb column blocks of BC columns sit on nb consecutive lanes (a
// "group"), lane s of the group owning columns s*BC+1 .. s*BC+BC on every row,
// and lane s sweeps row i = k - s in step k — a one-row skew per block — so the
// pair finishes in R + nb - 1 steps, with no carry buffer. Each step lane s
// takes from lane s-1 (DPP wave_shr:1; ignored on a group's first lane):
//   - the Y entering its first column on row i (lane s-1's row i, last step),
//   - the right-edge T of row i-1, its first diagonal (two steps back: held
//     one step in a register),
//   - on row R, the running sums ΣM, ΣX, so the final sums are accumulated
//     column by column left to right exactly as the reference does.
// A lane computes rows 1 .. R of its pair (pipeline fill / drain and a
// shorter pair's steps past its R are masked off).
// Block 0 starts `pad` = nb*BC - H columns left of column 1: those padding
// columns hold exact zeros (row 0's T is 0 left of column 0, so their M, X, Y
// and T stay 0 on every row, and column 0's T is T0 on row 0 and 0 below, as
// the reference's boundary), so the pair's last block ends exactly at column
// H and the last row's sums add only hap columns and leading +0.0 terms —
// the reference's sums, with no per-column mask.
// A lane's match window: columns c0+1 .. c0+64 of the hap's match table
// (rows of 32 bits, MSB first, kHapLead zero rows before), for each of the 5
// read codes, into its LDS slots mt[code * 64 + lane]. SPREAD (quad waves):
// the same 64 columns as 16 bytes, a group of four columns each
// (seg_spread.hpp), in the same region; padding columns left of column 1 and
// columns past the hap are zero bits in both forms.
template <bool SPREAD = false>
__device__ __forceinline__ void fill_window(uint2* __restrict__ mt, int lane, const LaneCtx& cx, int c0)
{
    const int H = cx.H;
    const int nwpad = (H + 31) / 32 + kHapLead;   // the trailing zero row
    const int w0 = (c0 >> 5) + kHapLead, r = c0 & 31;   // c0 >= -63 (block 0's padding): floor division
    const int i0 = min(w0, nwpad), i1 = min(w0 + 1, nwpad), i2 = min(w0 + 2, nwpad);
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const uint32_t h0 = hap_word(cx, i0 * 5 + c), h1 = hap_word(cx, i1 * 5 + c), h2 = hap_word(cx, i2 * 5 + c);
        const uint64_t x01 = (uint64_t(h0) << 32) | h1;
        const uint64_t x12 = (uint64_t(h1) << 32) | h2;
        const uint32_t m0 = uint32_t((x01 << r) >> 32), m1 = uint32_t((x12 << r) >> 32);
        if constexpr (SPREAD) {
            uint32_t* d = reinterpret_cast<uint32_t*>(mt) + spread_slot_off(c, lane) / 4;
            d[spread_group_off(0) / 4] = spread_nibbles(m0 >> 16);
            d[spread_group_off(4) / 4] = spread_nibbles(m0 & 0xffffu);
            d[spread_group_off(8) / 4] = spread_nibbles(m1 >> 16);
            d[spread_group_off(12) / 4] = spread_nibbles(m1 & 0xffffu);
        } else {
            mt[c * 64 + lane] = make_uint2(m0, m1);
        }
    }
}

// slut: the wave's prior tables in LDS. fp64: [ph2pr | pm | px | gapm]
// (load_slut); fp32: the pair table ptab (fill_ptab), which the constant-gap
// EQ path of the wide blocks (TAB) reads two columns at a time (cell_tab).
// QUAD (table widths of the fp32 EQ path only): slut is the workgroup's quad
// table, whose rows cover every quality of the wave's reads, and the window
// is kept spread.
template <typename T, int BC, bool CG, bool EQ, bool QUAD = false>
__device__ __forceinline__ void run_seg(const T* __restrict__ lut, const T* __restrict__ slut, const SegSteps& st,
                                        int lane, int s, const LaneCtx& cx, T T0, T& sumM, T& sumX,
                                        uint2* __restrict__ mt, uint32_t w1)
{
    constexpr int PD = seg_prefetch<T, BC>();
    constexpr bool TAB = std::is_same<T, float>::value && CG && EQ && BC >= kPtabMinWidth;
    static_assert(!QUAD || TAB, "the quad table is a form of the table path");
    constexpr int NP = BC / 2;   // column pairs of a row (block widths are even)
    static_assert(!TAB || BC % 2 == 0, "table priors come two columns at a time");
    const int pad = ((cx.H + BC - 1) / BC) * BC - cx.H;   // zero columns left of column 1 (block 0)
    int c0 = s * BC - pad;                                // this block: columns c0+1 .. c0+BC
    const int R = cx.R;
    // The two paths of a width start alike, and the window's addresses are
    // hoisted above the branch between them as far as they do, where they are
    // spilled once the paths' prologues differ. A text that differs per path
    // ends that at the first instruction.
    asm volatile("; run_seg CG=%1 QUAD=%2" : "+v"(c0) : "n"(int(CG)), "n"(int(QUAD)));
    fill_window<QUAD>(mt, lane, cx, c0);
    T Tt[BC], X[BC];
#pragma unroll
    for (int j = 0; j < BC; ++j) {
        Tt[j] = c0 + j + 1 >= 0 ? T0 : T(0);   // row 0: T0 from column 0 on, 0 on the padding left of it
        X[j] = T(0);
    }
    // wq[P]: the word of row i+1 (clamped to 1..R) at the steps of phase
    // P = (k-1) mod PD, for every lane at every step; the loads are issued
    // unconditionally so that each path has the same outstanding loads and
    // the wait for a word is the one PD steps after its load.
    // Row 1's word as the caller loaded it (w1). Loaded again here, its 64-bit
    // address stays live from the wave's prologue to the last path of the
    // width that loads it, through the step loops of the paths before: the
    // two registers the widest quad block does not have. Opaque, so that no
    // field of it is shared with the caller's uses of w1 (row0_t) and kept
    // from there to here (it was spilled).
    uint32_t wc = w1;
    asm volatile("" : "+v"(wc));
    uint32_t wq[PD];
#pragma unroll
    for (int P = 0; P < PD; ++P) wq[P] = row_word(cx, min(max(P + 2 - s, 1), R) - 1);
    RowConst<T> k;
    row_const<T>(lut, wc, row_word(cx, min(2, R) - 1), k);
    uint2 mrow{};
    if constexpr (!TAB) mrow = mt[k.rc * 64 + lane];
    // TAB: the table's LDS address, the coming row's table base and its first
    // entry (pair, or QUAD group of four), read at the end of the step before
    // (here: row 1's).
    // QUAD: the lane's slot of the spread window for the row's read code and
    // the byte of the row's second group ride along; mrow is unused.
    uint32_t tab_lds = 0, win_lds = 0;
    TabRow<TAB && QUAD> tr{};
    TabEnt<QUAD> pr0{};
    // TAB: what row w's cells start with. w's last uses are the window's slot
    // and the table base, and `after` (the index of the row word loaded next)
    // is ordered behind them, so that word can land in w's register.
    auto row_reads = [&](uint32_t w, int& after) {
        tr.base = tab_row<QUAD>(tab_lds, w);
        if constexpr (QUAD) {
            // (from the lane id each row, as the packed window's slot is: a
            // register held across the step loop is one the widest block lacks)
            tr.slot = win_lds + spread_slot_off(row_rc(w), lane);
            asm volatile("" : "+v"(after) : "v"(tr.slot), "v"(tr.base));
            pr0 = quad_read(tr.base, win_byte<0>(tr.slot));
            tr.byte = win_byte<1>(tr.slot);
        } else {
            const int mo = row_rc(w) * 64 + lane;
            asm volatile("" : "+v"(after) : "v"(mo), "v"(tr.base));
            tr.m = mt[mo];
            pr0 = ptab_pair<0>(tr.base, tr.m);
        }
    };
    if constexpr (TAB) {
        tab_lds = lds_addr(slut);
        if constexpr (QUAD) win_lds = lds_addr(mt);
        int none = 0;
        row_reads(wc, none);
    }
    // A pair's last block (and any lane past it) hands zeros to the lane on its
    // right, so a group's first lane needs no select: it receives Y = 0 entering
    // column 1 and T = 0 (column 0 below row 0) from its left neighbour, and
    // T0 (row 0's diagonal) from its own initial t_hold on row 1. Inside a
    // group, lane s-1's initial t_out is T0: lane s's row-1 diagonal.
    const uint32_t keep = (s + 1) * BC < cx.H ? 0xffffffffu : 0u;
    constexpr bool AND = BC * int(sizeof(T)) <= 128;   // masked's v_and form: fp32 up to 32 columns, fp64 16
    T y_out = T(0);                      // handed to lane s+1: Y past column c0+BC,
    T t_out = masked<AND>(T0, keep);     //   T[BC-1] of the last row
    T t_hold = c0 >= 0 ? T0 : T(0);      // lane s-1's right-edge T of the previous row (row 0: column c0's)
    // Running row sums (sumM, sumX): every lane adds its columns on every
    // sum-variant step and restarts from its left neighbour's at its last row
    // R; a lane stops at row R (rows past a pair's R feed nothing), so after
    // the sweep the pair's last block holds the pair's sums.
    auto step = [&](int kk, auto sum_tag, auto ph_tag) {
        constexpr bool SUM = decltype(sum_tag)::value;
        constexpr int P = decltype(ph_tag)::value;
        const int i = kk - s;
        const uint32_t wn = wq[P];   // row i+1, loaded PD steps ago
        T pm_n = T(0), px_n = T(0);
        uint2 m_n = mrow;
        // The word needed PD steps from now (row i + PD + 1). Not clamped to
        // the read: outside rows 1..R it feeds only rows no result depends on,
        // and the packed rows carry slack on both sides (engine.cpp o_rows).
        int ridx = i + PD;
        // TAB takes nothing of the next row yet: its match words, table base
        // and first pair are read at the end of the step, when the row's own
        // window is dead and gives them its registers (read here, they cost the
        // widest blocks the second pair in flight).
        if constexpr (CG && !TAB) {   // next row's prior constants (LDS) and match words
            const int qo = row_q(wn), mo = row_rc(wn) * 64 + lane;
            // Order the load after the last use of wn, so the word can land in
            // wn's register (no register move, hence no wait, at the loop back edge).
            asm volatile("" : "+v"(ridx) : "v"(qo), "v"(mo));
            pm_n = lds_pm(slut, qo);
            px_n = lds_px(slut, qo);
            m_n = mt[mo];
        } else if constexpr (!CG) {
            asm volatile("" : "+v"(ridx) : "v"(wn));
        }
        if constexpr (!TAB) wq[P] = row_word(cx, ridx);
        const T y_in = from_left(y_out);
        const T t_in = from_left(t_out);
        T sM_in = T(0), sX_in = T(0);
        if constexpr (SUM) {
            sM_in = from_left(sumM);
            sX_in = from_left(sumX);
        }
        // Row 1's diagonal is row 0's T at every column; below that, lane
        // s-1's right edge (column 0 for block 0: T[i][0] = 0 for i >= 1,
        // handed as 0 by the left neighbour, see keep).
        const T Tdiag = t_hold;
        const T Yl0 = y_in;   // block 0: Y[i][1] = 0*my + 0*yy = 0 (likewise)
        t_hold = t_in;
        if (unsigned(i - 1) < unsigned(R)) {   // this lane's rows 1 .. R of its pair
            if constexpr (!CG) {
                row_const<T>(lut, wc, wn, k);
                mrow = mt[k.rc * 64 + lane];   // reloaded every row: the cells below consume it
            }
            if (SUM && i == R) {
                sumM = s ? sM_in : T(0);
                sumX = s ? sX_in : T(0);
            }
            T Ml = T(0), Yl = Yl0;
            if constexpr (TAB) {
                constexpr int D = kPtabAhead;
                constexpr int NE = QUAD ? (BC + 3) / 4 : NP;   // table entries of a row
                static_assert(D == 2 && NE > D, "the ring holds two entries; a table row has more");
                TabEnt<QUAD> pr[D];
                pr[0] = pr0;
                if constexpr (QUAD) {
                    pr[1] = quad_read(tr.base, tr.byte);
                    tr.byte = win_byte<2>(tr.slot);
                } else {
                    pr[1] = ptab_pair<1>(tr.base, tr.m);
                }
                const float M0 = Tdiag * pr0.x;
                cell_tab<BC, 0, SUM, D, QUAD>(Tt, X, M0, Ml, Yl, pr, tr, k, sumM, sumX);
            } else {
                const T M0 = Tdiag * prior_next(mrow.x, k.pm, k.px);   // bit 31 of mrow.x first
                cell<T, BC, 0, BC, SUM, EQ>(Tt, X, M0, Ml, Yl, mrow.x, mrow.y, k.pm, k.px, k, 0, sumM, sumX);
            }
            y_out = masked<AND>(y_next<EQ>(Ml, Yl, k.my, k.yy), keep);
            t_out = masked<AND>(Tt[BC - 1], keep);
        }
        if constexpr (TAB) {
            // Unconditional, as below. wn's last uses are the window's slot and
            // the table base, so the word loaded now can land in wn's register.
            row_reads(wn, ridx);
            wq[P] = row_word(cx, ridx);
        } else if constexpr (CG) {
            // Unconditional (no register moves for a conditional update): a
            // lane before its row 1 takes row i + 1's constants too, and at
            // i = 0 those are row 1's, what it needs on its first row.
            k.pm = pm_n;
            k.px = px_n;
            mrow = m_n;   // a fresh window every step: the row's cells shifted the old one out
        }
        wc = wn;
    };
    // Everything the prologue loaded is in registers before the sweep: the
    // wait-count pass then sees only the sweep's own prefetches in flight and
    // waits on each word exactly PD steps after its load (s_waitcnt vmcnt(0)).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    // Groups of PD steps (phases 0..PD-1); the sum variant from the group that
    // holds step rmin on (extra steps past nsteps find every lane inactive).
    int kk = 1;
    int pk = st.prio ? 1 : INT32_MAX;   // next step at which the priority is updated (every 16 steps)
    for (; kk + PD - 1 < st.rmin; kk += PD) {
        if (kk >= pk) {
            set_prio(st.prio, kk, st.nsteps, st.t0);
            pk += 16;
        }
        for_phases<0, PD>([&](auto ph) { step(kk + decltype(ph)::value, std::false_type{}, ph); });
    }
    for (; kk <= st.nsteps; kk += PD) {
        if (kk >= pk) {
            set_prio(st.prio, kk, st.nsteps, st.t0);
            pk += 16;
        }
        for_phases<0, PD>([&](auto ph) { step(kk + decltype(ph)::value, std::true_type{}, ph); });
    }
}

// Whether every row of the wave's reads has a quality the quad table holds
// (kQuadQ0 .. kQuadQ0 + 63: bit 6 of (q - kQuadQ0) mod 128 clear). Lane s of a pair's nb lanes takes the rows 4s .. 4s + 3,
// 4(s + nb) .. of its read, eight 16-byte loads in flight (a load past the
// read's end repeats the first; the rows behind a read's last are there to
// load, part_setup.hpp row_pad_words, and are left out of the result).
typedef uint32_t rows4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ bool quad_scan(const LaneCtx& cx, int s, int nb)
{
    uint32_t high = 0;   // the OR of the rows' words less kQuadQ0: the low 7 bits are (q - kQuadQ0) mod 128
    const int last = cx.R - 1;
    constexpr int NL = 8;   // loads in flight
    for (int i = 4 * s; i <= last; i += 4 * NL * nb) {
        int at[NL];
        rows4 w[NL];
#pragma unroll
        for (int t = 0; t < NL; ++t) {
            at[t] = i + 4 * nb * t <= last ? i + 4 * nb * t : i;
            w[t] = *reinterpret_cast<const rows4*>(reinterpret_cast<const char*>(cx.rbase) +
                                                   (cx.rbyte + unsigned(at[t]) * 4u));
        }
#pragma unroll
        for (int t = 0; t < NL; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (at[t] + j <= last) high |= w[t][j] - uint32_t(kQuadQ0);
    }
    static_assert(kQuals == 2 * kQuadRows, "one bit tells the table's half of the qualities from the other");
    return __builtin_amdgcn_ballot_w64((high & uint32_t(kQuadRows)) != 0) == 0;
}

// Two compiled paths per width: EQ (the reference's constant 'I'/'I'/'+' gap
// qualities) and the generic per-row path (any gap qualities); the table
// widths of the fp32 EQ path a third, on the quad table qtab, for the waves
// whose qualities it holds.
template <typename T, int BC>
__device__ __forceinline__ void run_seg_bc(const T* __restrict__ lut, const T* __restrict__ slut, const SegSteps& st,
                                           int lane, int s, const LaneCtx& cx, T T0, T& sumM, T& sumX,
                                           uint2* __restrict__ mt, bool wave_eq, uint32_t w1,
                                           const T* __restrict__ qtab = nullptr)
{
    if constexpr (quad_width<T, BC>()) {
        if (wave_eq && quad_scan(cx, s, (cx.H + BC - 1) / BC)) {
            run_seg<T, BC, true, true, true>(lut, qtab, st, lane, s, cx, T0, sumM, sumX, mt, w1);
            return;
        }
    }
    if (wave_eq)
        run_seg<T, BC, true, true>(lut, slut, st, lane, s, cx, T0, sumM, sumX, mt, w1);
    else
        run_seg<T, BC, false, false>(lut, slut, st, lane, s, cx, T0, sumM, sumX, mt, w1);
}

// The fp64 rescue (intel_pairhmm.hpp:137-139) of the pairs this wave's fp32
// pass flagged (`todo`: their owner lanes). A wave with at most two, each with
// H <= kInWaveRescueMaxH, recomputes them itself while the rest of the pass
// runs — one pair at a time over the whole wave (8 columns per lane, the
// same run_seg in double) — so a batch with a few rescues (S2: ~2e-5 of
// the pairs) needs no separate latency-bound pass after the fp32 kernel. The
// others are appended to the rescue list for that pass.
// fp64 recompute of pair rp (slot rs) by the whole wave: 64 lanes of 8
// columns, raw f64 sum to the slot's record or raw64_zero[rp].
__device__ __forceinline__ void rescue_one(const LaneArgs& a, const PairDesc pd, int rp, int rs, int lane,
                                           uint2* __restrict__ mt)
{
    const int R = __builtin_amdgcn_readfirstlane(pd.y), H = __builtin_amdgcn_readfirstlane(pd.w);
    const int rx = __builtin_amdgcn_readfirstlane(pd.x);
    const LaneCtx cx{a.rows - kRowPadBefore, unsigned(rx + kRowPadBefore) * 4u, a.hapw,
                     unsigned(__builtin_amdgcn_readfirstlane(pd.z)) * 4u, R, H};
    constexpr int bc = seg64_width(0);
    const int nb = (H + bc - 1) / bc;
    const SegSteps st{R, R, R + nb - 1, 0};
    const uint32_t w1 = row_word(cx, 0);
    const double T0 = row0_t<double>(a.lut64, w1, H);
    const bool eq = read_eq(w1);
    double sM = 0.0, sX = 0.0;
    run_seg_bc<double, bc>(a.lut64, a.lut64, st, lane, lane, cx, T0, sM, sX, mt, eq, w1);
    if (lane == nb - 1) {
        const double r = sM + sX;
        if (a.rec) {   // record of slot rs: state and raw f64 (after the owner's store: same wave, program order)
            const unsigned long long b = (unsigned long long)__double_as_longlong(r);
            uint4* q = a.rec + rs;
            q->y = kRecInWave;
            *reinterpret_cast<uint2*>(&q->z) = make_uint2(unsigned(b), unsigned(b >> 32));
        } else {
            a.raw64_zero[rp] = r;
        }
    }
    __builtin_amdgcn_wave_barrier();   // the next pair rewrites mt
}

// Rescue pair rp (slot rs, hap length H) in this wave if it qualifies and the
// run's in-wave budget allows (wave-uniform), else append it to the fp64
// launch's list (lane `owner_lane`).
__device__ __forceinline__ void rescue_or_defer(const LaneArgs& a, bool few, int rp, int rs, int H, int R, int lane,
                                                int owner_lane, uint2* __restrict__ mt)
{
    bool here = few && H <= kInWaveRescueMaxH;
    if (here) {
        int c = 0;
        if (lane == 0) c = atomicAdd(a.inker_count, 1);
        here = __builtin_amdgcn_readfirstlane(c) < a.inker_limit;
    }
    if (here)
        rescue_one(a, a.sdesc[rs], rp, rs, lane, mt);   // sdesc[rs] = pairs[rp]
    else if (lane == owner_lane) {
        const int pos = atomicAdd(a.rescue_count, 1);
        a.rescue_list[pos] = rp;
        a.rescue_rh[pos] = pack_rh(R, H);
    }
}

__device__ __forceinline__ void rescue_in_wave(const LaneArgs& a, uint64_t todo, int pid, int slot, int H, int R,
                                               int lane, uint2* __restrict__ mt)
{
    // (No fp64 launch after this pass: every one, the list would go unread.)
    const bool few = a.inker_count != nullptr && (a.solo_counters != nullptr || __popcll(todo) <= 2);
    // The owners' result records are complete before a rescue rewrites part
    // of one (the same address from another lane of this wave).
    if (a.rec) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        rescue_or_defer(a, few, __builtin_amdgcn_readlane(pid, l), __builtin_amdgcn_readlane(slot, l),
                        __builtin_amdgcn_readlane(H, l), __builtin_amdgcn_readlane(R, l), lane, l, mt);
    }
}

}  // namespace seg
}  // namespace hcphmm
