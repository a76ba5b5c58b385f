// Device side of the read preparation (include/hc_prep.h): the launch record
// shared by prep_kernels.hip and prep_engine.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "prep_body.hpp"

namespace hcprep {

constexpr int kPrepWavesPerBlock = 4;   // one wave per window

struct PrepArgs {
    const PrepWindow* windows;
    int32_t n_windows;
    const PrepRead* reads;
    const uint32_t* words;
    hc_prep_record* records;      // per read, pool order
    int32_t* kept;                // per window at its first_read: the kept reads' indices, input order
    int32_t* n_kept;              // per window
    int64_t* kept_bases;          // per window
    unsigned long long* err;      // kNoError, or min of read * 8 + PrepError
};

hipError_t launch_prep(const PrepArgs& a, hipStream_t st);

}  // namespace hcprep
