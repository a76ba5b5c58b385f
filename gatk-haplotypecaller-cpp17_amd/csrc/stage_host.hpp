// Host plumbing shared by the eight stage engines (sw_engine.cpp, gt_engine.cpp,
// region_engine.cpp, asm_engine.cpp, prep_engine.cpp, sam_engine.cpp,
// contig_engine.cpp, genome_engine.cpp) and the window caller that chains them (call_engine.cpp):
// the error return, 256-byte rounding, the offset carver, grow-only device /
// pinned buffers, the phase trace, the HIP_TRY macro, the Stage (an engine's
// lock, stream, once-only setup and buffers, released by hc_phmm_shutdown
// through release_all) and the frame of an entry point that returns a result
// object. Host only: no .hip file includes it. The PairHMM engine's pooled,
// multi-device buffers (engine_core.hpp) are a different design.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/hc_pairhmm.h"

namespace hcphmm {
void set_last_error(const std::string& msg);
int primary_device();
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
    void count(const char* what, long long x)   // a whole number, printed as one
    {
        if (on) line += std::string(" ") + what + "=" + std::to_string(x);
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

struct Stage;
// Every Stage of the library, in the order they were constructed (at load time), and
// what hc_phmm_shutdown does with them (stage_host.cpp).
std::vector<Stage*>& stages();
void release_all();

// What an engine owns on the device: its lock (held for the whole of every entry
// point), its stream, a once-only setup with its teardown, and its buffers.
struct Stage {
    std::mutex mu;
    hipStream_t stream = nullptr;   // stays null in a stage whose kernels run on another stage's stream
    bool ready = false;             // stream and setup are complete

    // setup runs once behind the stream's creation and returns 0 or an error with
    // its message set; teardown undoes it and must be safe after a setup that failed half way.
    Stage(std::initializer_list<Buf*> bufs, bool own_stream = true, int (*setup)(hipStream_t) = nullptr,
          void (*teardown)() = nullptr)
        : bufs_(bufs), own_stream_(own_stream), setup_(setup), teardown_(teardown)
    {
        stages().push_back(this);
    }
    // Further buffers that this stage's lock guards and its release drops.
    Stage& with(std::initializer_list<Buf*> bufs)
    {
        bufs_.insert(bufs_.end(), bufs);
        return *this;
    }

    // With the lock held. The PairHMM engine is initialised (an implicit init picks
    // the device and leaves the caller's mode alone), its first device is current on
    // the calling thread, and stream and setup are ready. A failure leaves nothing
    // behind: the next call starts over.
    int ensure_init(int device = -1)
    {
        if (int rc = hc_phmm_init(HC_PHMM_FLAG_KEEP_MODE, device)) return rc;
        const hipError_t e = hipSetDevice(hcphmm::primary_device());
        if (e != hipSuccess) return hip_fail(stream, "hipSetDevice(hcphmm::primary_device())", e);
        if (ready) return HC_PHMM_OK;
        int rc = HC_PHMM_OK;
        if (own_stream_ && !stream) {
            const hipError_t es = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
            if (es != hipSuccess) rc = hip_fail(stream = nullptr, "hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)", es);
        }
        if (!rc && setup_) rc = setup_(stream);
        if (rc) close();
        ready = !rc;
        return rc;
    }

    // hc_phmm_shutdown: the next call re-creates everything on whatever device the
    // engine is then initialised on.
    void release()
    {
        std::lock_guard<std::mutex> lk(mu);
        close();
    }

private:
    void close()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        if (teardown_) teardown_();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        ready = false;
        for (Buf* b : bufs_) drop(*b);
    }
    std::vector<Buf*> bufs_;
    const bool own_stream_;
    int (*const setup_)(hipStream_t);
    void (*const teardown_)();
};

// The frame of an entry point that hands out a result object, with the engine's
// lock held: null check, a fresh R for body(R&) to fill, *out set only on success.
// A host allocation that fails drains *drain (null: no stream of its own to drain).
template <class R, class F>
int call_frame(R** out, const hipStream_t* drain, F&& body)
{
    if (!out) return fail(HC_PHMM_EINVAL, "null out");
    *out = nullptr;
    try {
        std::unique_ptr<R> res(new R());
        if (int rc = body(*res)) return rc;
        *out = res.release();
        return HC_PHMM_OK;
    } catch (const std::bad_alloc&) {
        if (drain && *drain) (void)hipStreamSynchronize(*drain);
        return fail(HC_PHMM_ENOMEM, "host allocation failed");
    }
}

}  // namespace stage_host
