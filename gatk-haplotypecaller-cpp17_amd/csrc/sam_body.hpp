// One SAM alignment line to a record (include/hc_sam.h): operator>>(istream&,
// SAMRecord&) and Cigar::to_cigar_elements (sam/sam.hpp:100-114,
// sam/cigar.hpp:57-68) on a byte range [begin, end) of the text, with the
// syntax checks the reference leaves out.
//
// A line is read 64 bytes at a time. What is written here, once, is everything
// that does not depend on how the 64-bit masks of a row come about: the token
// starts and ends from the "not whitespace" mask (sam_token_masks, sam_tokens),
// one CIGAR element from its operator's position (sam_element), the numeric
// fields (sam_numeric) and the record with its error and defect codes
// (sam_record). sam_kernels.hip makes the masks by wave ballots, one wave per
// line; with SAMX_HOST_ONLY (no HIP header) tests/cpp/sam_host_main.cpp makes
// them with a loop over 64 bytes and runs the same functions under the host
// sanitizers. No byte at or past `end` is read, and `end` never exceeds the
// text's length.
#pragma once
#ifdef SAMX_HOST_ONLY
#define SAMX_FN
#else
#include <hip/hip_runtime.h>
#define SAMX_FN __host__ __device__
#endif

#include <cstdint>

#include "../../include/hc_sam.h"

namespace hcsam {

// Syntax errors, by precedence within one line. The error word is min over
// lines of (0-based line index) * 16 + code.
enum SamError : int32_t {
    kErrNone = 0,
    kErrFields = 1,   // 1 to 10 fields
    kErrFlag = 2,
    kErrPos = 3,
    kErrMapq = 4,
    kErrCigar = 5,
    kErrPnext = 6,
    kErrTlen = 7,
    kErrLong = 8,     // a line of 2^31 bytes or more
    kSkip = -1        // no field at all: the line has no record
};
constexpr unsigned long long kNoError = ~0ull;

constexpr uint32_t kReadOps = 0x193u;   // M I S = X   (Cigar::get_read_length)
constexpr int kFields = 11;

// The C locale's isspace: ' ' and \t \n \v \f \r.
SAMX_FN inline bool sam_space(uint8_t c) { return c == 32u || (c >= 9u && c <= 13u); }
SAMX_FN inline bool sam_digit(uint8_t c) { return uint32_t(c) - 48u <= 9u; }

SAMX_FN inline int sam_ctz(uint64_t m)
{
#ifdef SAMX_HOST_ONLY
    return __builtin_ctzll(m);
#else
#ifdef __HIP_DEVICE_COMPILE__
    return __ffsll(static_cast<unsigned long long>(m)) - 1;
#else
    return __builtin_ctzll(m);
#endif
#endif
}

// Of one row of 64 bytes: bit l of `nonws` says byte l is inside the line and
// not whitespace, `carry` that the byte before the row was. A token starts
// where a set bit follows a clear one and ends (exclusive) where a clear bit
// follows a set one; a byte past the line's end is a clear bit.
SAMX_FN inline void sam_token_masks(uint64_t nonws, uint64_t carry, uint64_t& starts, uint64_t& ends)
{
    const uint64_t prev = (nonws << 1) | carry;
    starts = nonws & ~prev;
    ends = ~nonws & prev;
}

// Token bounds of a line as offsets from its first byte: tok[f] the start and
// tok[kFields + f] the end of field f. Fed row by row (`off` = the row's
// offset); done() once the eleventh token has ended. `tok` has 2 * kFields
// entries; on the device it is the wave's LDS row and every lane stores the
// same values, so a lane only ever reads what it wrote itself.
struct SamTokens {
    int32_t* tok;
    int32_t n_start = 0, n_end = 0;
    uint64_t carry = 0;
    SAMX_FN explicit SamTokens(int32_t* where) : tok(where) {}
    SAMX_FN bool done() const { return n_end >= kFields; }
    SAMX_FN void row(uint64_t nonws, int32_t off)
    {
        uint64_t starts, ends;
        sam_token_masks(nonws, carry, starts, ends);
        carry = nonws >> 63;
        for (; starts && n_start < kFields; starts &= starts - 1) tok[n_start++] = off + sam_ctz(starts);
        for (; ends && n_end < kFields; ends &= ends - 1) tok[kFields + n_end++] = off + sam_ctz(ends);
    }
    // After the last row: a token that runs to the line's last byte ends with the line.
    SAMX_FN void finish(int32_t len)
    {
        if (n_end < kFields && carry) tok[kFields + n_end++] = len;
    }
};

// Decimal digits only, value <= max.
SAMX_FN inline bool sam_unsigned(const uint8_t* t, int64_t b, int64_t e, uint64_t max, uint64_t& v)
{
    v = 0;
    for (int64_t i = b; i < e; ++i) {
        if (!sam_digit(t[i])) return false;
        v = v * 10u + (uint32_t(t[i]) - 48u);
        if (v > max) return false;
    }
    return e > b;
}

// The numeric field j of a tokenised line: 0 FLAG, 1 POS, 2 MAPQ, 3 PNEXT, 4 TLEN.
SAMX_FN inline bool sam_numeric(const uint8_t* t, int64_t begin, const int32_t* tok, int j, uint64_t& v)
{
    const int f = j == 0 ? 1 : j == 1 ? 3 : j == 2 ? 4 : j == 3 ? 7 : 8;
    const int64_t b = begin + tok[f], e = begin + tok[kFields + f];
    if (j == 4) {
        const bool neg = t[b] == '-';
        return sam_unsigned(t, b + (neg ? 1 : 0), e, neg ? 0x80000000u : 0x7fffffffu, v);
    }
    return sam_unsigned(t, b, e, (j == 0 || j == 2) ? 0xffffu : 0xffffffffu, v);
}

SAMX_FN inline int32_t sam_op(uint8_t c)
{
    switch (c) {
        case 'M': return 0;
        case 'I': return 1;
        case 'D': return 2;
        case 'N': return 3;
        case 'S': return 4;
        case 'H': return 5;
        case 'P': return 6;
        case '=': return 7;
        case 'X': return 8;
        default: return -1;
    }
}

// The CIGAR element whose operator is the byte at `i` (a byte of the token that
// is not a digit): its digits are read backwards down to the token's start `b`.
// False for an unknown operator, no digit in front of it or a length above
// HC_SAM_MAX_CIGAR_LENGTH.
SAMX_FN inline bool sam_element(const uint8_t* t, int64_t b, int64_t i, uint32_t& word, uint64_t& read_len)
{
    const int32_t op = sam_op(t[i]);
    if (op < 0 || i == b || !sam_digit(t[i - 1])) return false;
    uint64_t len = 0, place = 1;
    for (int64_t j = i - 1; j >= b && sam_digit(t[j]); --j) {
        const uint64_t d = uint32_t(t[j]) - 48u;
        if (d && place > 100000000u) return false;   // a non-zero digit in the tenth place or beyond
        len += d * place;
        if (place <= 100000000u) place *= 10u;
    }
    if (len > HC_SAM_MAX_CIGAR_LENGTH) return false;
    word = uint32_t(len) << 4 | uint32_t(op);
    read_len = ((kReadOps >> op) & 1u) ? len : 0;
    return true;
}

// The record of a line with eleven tokens, or its syntax error. num_ok: bit j
// says sam_numeric(j) succeeded, val[j] its value. o.cigar is the CIGAR token's
// offset from `begin` (the emit pass turns it into the pool index).
SAMX_FN inline int32_t sam_record(const uint8_t* t, int64_t begin, const int32_t* tok, uint32_t num_ok, const uint64_t* val,
                                  bool cigar_ok, int32_t n_cigar, uint64_t read_len, hc_sam_record& o)
{
    o = hc_sam_record{};
    o.line = begin;
    if (!(num_ok & 1u)) return kErrFlag;
    if (!(num_ok & 2u)) return kErrPos;
    if (!(num_ok & 4u)) return kErrMapq;
    if (!cigar_ok) return kErrCigar;
    if (!(num_ok & 8u)) return kErrPnext;
    if (!(num_ok & 16u)) return kErrTlen;
    o.flag = uint16_t(val[0]);
    o.pos = uint32_t(val[1]);
    o.mapq = uint16_t(val[2]);
    o.n_cigar = n_cigar;
    o.cigar = tok[5];
    o.mate_same_contig = (tok[kFields + 6] - tok[6] == 1 && t[begin + tok[6]] == '=') ? 1 : 0;
    o.seq_off = uint32_t(tok[9]);
    o.seq_len = tok[kFields + 9] - tok[9];
    o.qual_off = uint32_t(tok[10]);
    o.qual_len = tok[kFields + 10] - tok[10];
    o.defect = o.pos == 0                              ? HC_SAM_DEFECT_POS_ZERO
               : o.n_cigar == 0                        ? HC_SAM_DEFECT_NO_CIGAR
               : read_len != uint64_t(o.seq_len)       ? HC_SAM_DEFECT_CIGAR_LENGTH
               : o.qual_len != o.seq_len               ? HC_SAM_DEFECT_QUAL_LENGTH
               : o.seq_len > HC_PHMM_MAX_READ_LEN      ? HC_SAM_DEFECT_TOO_LONG
                                                       : HC_SAM_DEFECT_NONE;
    return kErrNone;
}

// Where line `k` of `n_lines` ends (its '\n' excluded); starts[k + 1] is read only for k + 1 < n_lines.
SAMX_FN inline int64_t sam_line_end(const uint8_t* t, int64_t len, const int64_t* starts, int64_t k, int64_t n_lines)
{
    if (k + 1 < n_lines) return starts[k + 1] - 1;
    return t[len - 1] == '\n' ? len - 1 : len;
}

}  // namespace hcsam
