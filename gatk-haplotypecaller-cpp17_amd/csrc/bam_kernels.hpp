// Device side of the BAM front (include/hc_bam.h): the launch records shared by
// bam_kernels.hip and bam_engine.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hc_bam.h"
#include "bgzf_body.hpp"

namespace hcbam {

constexpr int kWavesPerBlock = 4;
constexpr unsigned long long kNoError = ~0ull;
constexpr int kErrCigarOp = 1;   // the decode kernel's only error: record * 16 + kErrCigarOp

struct InflateArgs {
    const uint8_t* file;                 // the compressed file on the device
    const hcbgzf::BgzfMember* members;
    int32_t n_members;
    uint8_t* out;                        // 256-byte aligned; member m's bytes at out + members[m].out_off
    int32_t* err;                        // per member: hcbgzf::BgzfError
};

// Offsets of a record's fields from its block_size word.
constexpr int kRefId = 4, kPos = 8, kLName = 12, kMapq = 13, kNCigar = 16, kFlag = 18, kLSeq = 20, kNextRefId = 24, kName = 36;

struct DecodeArgs {
    const uint8_t* stream;        // the inflated bytes
    const int64_t* rec_off;       // per record: its block_size word, the whole record inside the stream (the host's walk)
    const int64_t* cigar_first;   // n_records + 1: the exclusive sum of n_cigar_op
    const int64_t* bases_first;   // n_records + 1: the exclusive sum of 2 * l_seq
    int32_t n_records;
    hc_sam_record* records;
    int32_t* line_no;             // the 1-based ordinal
    int32_t* ref_id;
    uint32_t* pool;
    uint8_t* bases;
    unsigned long long* err;
};

hipError_t launch_inflate(const InflateArgs& a, hipStream_t st);
hipError_t launch_crc(const InflateArgs& a, hipStream_t st);
hipError_t launch_decode(const DecodeArgs& a, hipStream_t st);
// contig_of[k] = ref_id[k] < 0 ? -1 : ref_contig[ref_id[k]]
hipError_t launch_contig_of(const int32_t* ref_id, const int32_t* ref_contig, int32_t n_records, int32_t* contig_of,
                            hipStream_t st);

}  // namespace hcbam
