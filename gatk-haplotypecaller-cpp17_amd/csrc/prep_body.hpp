// Read preparation for one read (include/hc_prep.h): the four flag filters,
// ReadClipper::revert_soft_clipped_bases, hard_clip_to_interval and the
// minimum-length filter (utils/read_filter.hpp, utils/read_clipper.hpp:32-91),
// on (offset, length) views instead of strings.
//
// Written once: the body of prep_kernel (one lane per read) and, with
// PREPX_HOST_ONLY (no HIP header), of the host program that
// tests/cpp/prep_host_main.cpp checks under the host sanitizers.
//
// Widths are the reference's: POS is uint32 (sam.hpp:22), everything that meets
// a CigarElement length or an Interval bound is size_t, here uint64_t.
#pragma once
#ifdef PREPX_HOST_ONLY
#define PREPX_FN
#else
#include <hip/hip_runtime.h>
#define PREPX_FN __host__ __device__
#endif

#include <cstdint>

#include "../../include/hc_prep.h"

namespace hcprep {

// What the device reads per read; cigar_off indexes the call's word pool.
struct PrepRead {
    int64_t cigar_off;
    uint32_t pos;
    int32_t seq_len;
    int32_t n_cigar;
    uint16_t flag, mapq;
    uint32_t mate_same_contig;
    uint32_t pad;
};

struct PrepWindow {
    int64_t padded_begin, padded_end;
    int64_t first_read;   // index of the window's first read in the call's read pool
    int32_t n_reads;
    int32_t pad;
};

// Device-side input errors, by precedence within one read. The error word is
// min over reads of (pool index of the read) * 8 + code.
enum PrepError : int32_t { kErrNone = 0, kErrPosZero = 1, kErrNoCigar = 2, kErrOp = 3, kErrLength = 4 };
constexpr unsigned long long kNoError = ~0ull;

constexpr uint32_t kOpM = 0, kOpS = 4, kOpMax = 8;
constexpr uint32_t kRefOps = 0x18Du;    // M D N = X   (Cigar::get_reference_length)
constexpr uint32_t kReadOps = 0x193u;   // M I S = X   (Cigar::get_read_length)

// Fills `o` and returns kErrNone, or returns the input error of a read that
// passes the flag filters (`o` is then a dropped, untouched read).
PREPX_FN inline int32_t prep_one(const PrepRead& r, const uint32_t* words, uint64_t win_begin, uint64_t win_end,
                                 hc_prep_record& o)
{
    o.begin = o.end = 0;
    o.new_pos = r.pos;
    o.offset = 0;
    o.length = r.seq_len;
    o.keep = 0;
    o.front_to_M = o.back_to_M = 0;
    o.drop_reason = r.mapq < HC_PREP_MIN_MAPQ ? HC_PREP_DROP_MAPQ
                    : (r.flag & 0x400)        ? HC_PREP_DROP_DUPLICATE
                    : (r.flag & 0x100)        ? HC_PREP_DROP_SECONDARY
                    : !r.mate_same_contig     ? HC_PREP_DROP_MATE_CONTIG
                                              : HC_PREP_KEPT;
    if (o.drop_reason != HC_PREP_KEPT) return kErrNone;
    o.drop_reason = HC_PREP_DROP_MIN_LENGTH;   // until the read is kept: an input error leaves it dropped
    if (r.pos == 0) return kErrPosZero;
    if (r.n_cigar <= 0) return kErrNoCigar;

    // one walk over the words
    uint64_t ref_len = 0, read_len = 0;
    bool bad_op = false;
    for (int32_t i = 0; i < r.n_cigar; ++i) {
        const uint32_t w = words[i], op = w & 15u;
        const uint64_t len = w >> 4;
        bad_op |= op > kOpMax;
        if ((kRefOps >> op) & 1u) ref_len += len;
        if ((kReadOps >> op) & 1u) read_len += len;
    }
    if (bad_op) return kErrOp;
    if (read_len != uint64_t(r.seq_len)) return kErrLength;

    const uint64_t front_len = words[0] >> 4, back_len = words[r.n_cigar - 1] >> 4;
    const uint32_t front_op = words[0] & 15u;
    uint32_t back_op = words[r.n_cigar - 1] & 15u;
    uint64_t off = 0, size = uint64_t(r.seq_len);
    uint32_t pos = r.pos;

    // revert_soft_clipped_bases
    if (r.flag & 0x10) {
        if (front_op == kOpS) {
            off += front_len;
            size -= front_len;
        }
        if (back_op == kOpS) {
            o.back_to_M = 1;
            ref_len += back_len;
        }
    } else {
        const uint32_t alignment_begin = pos - 1u;
        if (front_op == kOpS && uint64_t(alignment_begin) >= front_len) {
            o.front_to_M = 1;
            ref_len += front_len;
            pos = uint32_t(uint64_t(alignment_begin) - front_len + 1u);
            if (r.n_cigar == 1) back_op = kOpM;   // back() is the element just rewritten
        }
        if (back_op == kOpS) size -= back_len;
    }

    // hard_clip_to_interval
    const uint64_t alignment_begin = uint64_t(uint32_t(pos - 1u));
    const uint64_t alignment_end = alignment_begin + ref_len;
    if (alignment_begin < win_begin) {
        uint64_t clip = win_begin - alignment_begin;
        if (clip > size) clip = size;
        off += clip;
        size -= clip;
    }
    if (alignment_end > win_end) {
        const uint64_t clip = alignment_end - win_end;
        if (clip <= size) size -= clip;   // size - clip wraps otherwise: substr(0, huge) keeps the read whole
    }

    o.begin = int64_t(alignment_begin);
    o.end = int64_t(alignment_end);
    o.new_pos = pos;
    o.offset = int32_t(off);
    o.length = int32_t(size);
    if (size >= HC_PREP_MIN_LENGTH) {
        o.keep = 1;
        o.drop_reason = HC_PREP_KEPT;
    }
    return kErrNone;
}

}  // namespace hcprep
