// Device side of the SAM parser (include/hc_sam.h): the launch record shared by
// sam_kernels.hip and sam_engine.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "sam_body.hpp"

namespace hcsam {

constexpr int kChunkBytes = 1024;      // one wave: 64 lanes x 16 bytes
constexpr int kWavesPerBlock = 4;
constexpr int32_t kNoHeaderEnd = 0x7f7f7f7f;   // what a 0x7F memset leaves: every line so far began with '@'

struct SamArgs {
    const uint8_t* text;        // allocated up to a multiple of kChunkBytes; bytes at and past `len` are never used
    int64_t len;
    int64_t n_chunks;
    int32_t* chunk_lines;       // per chunk: the lines that start in it
    const int64_t* chunk_first; // its exclusive scan
    int64_t* line_start;        // per line
    int32_t n_lines;
    int32_t* header_end;        // kNoHeaderEnd, or the smallest index of a line whose first byte is not '@'
    unsigned long long* err;    // kNoError, or min of line * 16 + SamError
    hc_sam_record* tmp;         // per line, cigar = the token's offset
    int32_t* has_record;        // per line: 0 / 1
    int32_t* n_words;           // per line
    const int64_t* rec_first;   // exclusive scans of the two
    const int64_t* word_first;
    hc_sam_record* records;     // per record
    int32_t* line_no;           // per record: 1-based line
    uint32_t* pool;
};

hipError_t launch_line_count(const SamArgs& a, hipStream_t st);
hipError_t launch_line_write(const SamArgs& a, hipStream_t st);
hipError_t launch_parse(const SamArgs& a, hipStream_t st);
hipError_t launch_emit(const SamArgs& a, hipStream_t st);
// out[0 .. n]: the exclusive scan of in[0 .. n) and, at out[n], the total. Three
// launches; `work` holds scan_work_bytes(n) bytes and is free again when they are done.
constexpr int kScanBlock = 1024, kScanPer = 4, kScanTile = kScanBlock * kScanPer;
inline int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }
inline size_t scan_work_bytes(int64_t n) { return sizeof(int64_t) * size_t(2 * scan_tiles(n) + 1); }
hipError_t launch_scan(const int32_t* in, int64_t n, int64_t* out, int64_t* work, hipStream_t st);

}  // namespace hcsam
