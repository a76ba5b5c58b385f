// Host plumbing shared by the stage engines (sw_engine.cpp, gt_engine.cpp,
// region_engine.cpp, asm_engine.cpp): the error return, 256-byte rounding, the
// offset carver, grow-only device / pinned buffers, the phase trace and the
// HIP_TRY macro. Host only: no .hip file includes it. The PairHMM engine's
// pooled, multi-device buffers (engine_core.hpp) are a different design.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/hc_pairhmm.h"

namespace hcphmm {
void set_last_error(const std::string& msg);
}

namespace stage_host {

inline int fail(int code, const std::string& msg)
{
    hcphmm::set_last_error(msg);
    return code;
}

inline size_t up(size_t x) { return (x + 255) & ~size_t(255); }

// Carves consecutive 256-byte aligned pieces (an empty piece still gets its own address).
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t at = off;
        off = up(off + std::max<size_t>(bytes, 1));
        return at;
    }
};

// Grow-only buffer, device or pinned; its owner's lock guards it.
struct Buf {
    char* p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
};

inline void drop(Buf& b)
{
    if (b.p) (void)(b.pinned ? hipHostFree(b.p) : hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
}

// At least `bytes`: grows by a quarter, frees before it allocates. `what` is the
// text of the HC_PHMM_ENOMEM (== HC_SW_ENOMEM) error.
inline int reserve(Buf& b, size_t bytes, const char* what)
{
    if (bytes <= b.bytes) return HC_PHMM_OK;
    drop(b);
    const size_t want = bytes + bytes / 4;
    const hipError_t e = b.pinned ? hipHostMalloc(reinterpret_cast<void**>(&b.p), want, hipHostMallocDefault)
                                  : hipMalloc(reinterpret_cast<void**>(&b.p), want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(HC_PHMM_ENOMEM, what);
    }
    b.bytes = want;
    return HC_PHMM_OK;
}

// <env>=1: host wall clock of a call's phases on stderr (ms since the call began),
// one line "<prefix> name=value ..." when the call ends.
struct Trace {
    bool on = false;
    const char* prefix;
    std::chrono::steady_clock::time_point t0;
    std::string line;
    Trace(const char* env, const char* prefix_) : prefix(prefix_)
    {
        const char* e = std::getenv(env);
        on = e && e[0] == '1';
        if (on) t0 = std::chrono::steady_clock::now();
    }
    void mark(const char* what)
    {
        if (on) value(what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    void value(const char* what, double x)
    {
        if (!on) return;
        char tmp[64];
        std::snprintf(tmp, sizeof(tmp), " %s=%.3f", what, x);
        line += tmp;
    }
    ~Trace()
    {
        if (on) std::fprintf(stderr, "%s%s\n", prefix, line.c_str());
    }
};

// A failed HIP call: drains `st` (a null stream is left alone) so that no copy is
// still reading or writing a pinned block the next call reuses, then sets the message.
inline int hip_fail(hipStream_t st, const char* expr, hipError_t e)
{
    if (st) (void)hipStreamSynchronize(st);
    return fail(HC_PHMM_EHIP, std::string(expr) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(st, expr)                                                     \
    do {                                                                      \
        hipError_t e_ = (expr);                                               \
        if (e_ != hipSuccess) return stage_host::hip_fail((st), #expr, e_);   \
    } while (0)

}  // namespace stage_host
