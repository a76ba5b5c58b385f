// What the contig caller (contig_engine.cpp) and the genome caller
// (genome_engine.cpp) share with the SAM parser (sam_engine.cpp): a parse that
// leaves its records and the text on the device and hands the parser's lock to
// the caller. The BAM front (bam_engine.cpp) fills the same result object from
// its own kernels, under the parser's lock and on the parser's stream, and sends
// its file up through the parser's staging block.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/hc_sam.h"
#include "stage_host.hpp"

struct hc_sam_result {
    std::vector<hc_sam_record> records;
    std::vector<int32_t> line_no;
    std::vector<uint32_t> pool;
    int32_t n_header_lines = 0;
};

namespace hcsam {

struct Resident {
    hipStream_t stream = nullptr;            // the parser's stream; the records are complete on it
    const hc_sam_record* records = nullptr;  // device
    const int32_t* line_no = nullptr;        // device
    int32_t n_records = 0;
    const uint8_t* text = nullptr;           // device: the text the records' `line` offsets point into
    int64_t text_len = 0;
};

// hc_sam_parse. On success `lk` owns the parser's lock and `dev` names the
// records and the text on the device; they stay as they are until `lk` is released.
int parse_resident(const uint8_t* text, int64_t text_len, hc_sam_result** out, std::unique_lock<std::mutex>& lk,
                   Resident& dev);

// The parser's lock, stream and buffers.
stage_host::Stage& parser_stage();
// With the parser's lock held and the stage initialised: `bytes` to the device
// through the pinned staging block of HC_SAM_STAGE_BYTES, piece after piece, into
// the parser's text buffer of at least `room` >= len bytes.
int upload(const uint8_t* bytes, int64_t len, size_t room, const uint8_t*& on_device);
// The same for stretches of host bytes that lie apart: they are packed one behind
// the other in the staging block itself, `total` bytes in all, with no copy in between.
struct Piece {
    const uint8_t* bytes;
    int64_t len;
};
int upload_pieces(const Piece* pieces, size_t n_pieces, int64_t total, size_t room, const uint8_t*& on_device);

}  // namespace hcsam
