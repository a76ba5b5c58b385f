// What the contig caller (contig_engine.cpp) and the genome caller
// (genome_engine.cpp) share with the SAM parser (sam_engine.cpp): a parse that
// leaves its records and the text on the device and hands the parser's lock to
// the caller.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/hc_sam.h"

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

}  // namespace hcsam
