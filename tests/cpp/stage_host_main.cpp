// csrc/stage_host.hpp alone (tests/test_stage_host.py): Stage, release_all and
// call_frame with the HIP runtime and the PairHMM engine replaced by the stubs
// below, so that the failure paths of ensure_init run without a device.
#include "../../gatk-haplotypecaller-cpp17_amd/csrc/stage_host.hpp"

#include <cassert>
#include <cstdio>
#include <cstdlib>

static int g_init_rc = 0, g_init_flags = -1;
static int g_streams_made = 0, g_streams_gone = 0, g_syncs = 0;
static bool g_stream_create_fails = false, g_setdevice_fails = false;
static int g_allocs = 0;
static std::string g_err;

extern "C" int hc_phmm_init(uint32_t flags, int) { g_init_flags = int(flags); return g_init_rc; }
namespace hcphmm {
int primary_device() { return 0; }
void set_last_error(const std::string& m) { g_err = m; }
}
extern "C" {
hipError_t hipSetDevice(int) { return g_setdevice_fails ? hipErrorInvalidDevice : hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned)
{
    if (g_stream_create_fails) return hipErrorOutOfMemory;
    *s = reinterpret_cast<hipStream_t>(std::malloc(8));
    ++g_streams_made;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { ++g_syncs; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { std::free(s); ++g_streams_gone; return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) { *p = std::malloc(n); ++g_allocs; return hipSuccess; }
hipError_t hipFree(void* p) { std::free(p); --g_allocs; return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = std::malloc(n); ++g_allocs; return hipSuccess; }
hipError_t hipHostFree(void* p) { std::free(p); --g_allocs; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub error"; }
}

using namespace stage_host;

static Buf b1, b2{nullptr, 0, true}, b3;
static void* g_table = nullptr;
static bool g_setup_fails = false;
static int g_teardowns = 0;
static Stage st({&b1, &b2}, true,
                [](hipStream_t s) -> int {
                    HIP_TRY(s, hipMalloc(&g_table, 64));
                    if (g_setup_fails) return fail(HC_PHMM_EHIP, "setup failed");
                    return HC_PHMM_OK;
                },
                [] {
                    if (g_table) (void)hipFree(g_table);
                    g_table = nullptr;
                    ++g_teardowns;
                });
static Stage nostream({&b3}, false);

struct Res { std::vector<int> v; };

int main()
{
    assert(stages().size() == 2);
    // the engine's init fails: passed through, nothing made
    g_init_rc = HC_PHMM_ENODEV;
    assert(st.ensure_init() == HC_PHMM_ENODEV && !st.stream && !st.ready && g_streams_made == 0);
    g_init_rc = 0;
    assert(g_init_flags == int(HC_PHMM_FLAG_KEEP_MODE));
    // hipSetDevice fails
    g_setdevice_fails = true;
    assert(st.ensure_init() == HC_PHMM_EHIP && !st.stream && !st.ready);
    g_setdevice_fails = false;
    // the stream cannot be made
    g_stream_create_fails = true;
    assert(st.ensure_init() == HC_PHMM_EHIP && !st.stream && !st.ready);
    g_stream_create_fails = false;
    // the setup fails after its allocation: table and stream are undone, the next call starts over
    g_setup_fails = true;
    assert(st.ensure_init() == HC_PHMM_EHIP && g_err == "setup failed");
    assert(!st.stream && !st.ready && !g_table && g_streams_made == 1 && g_streams_gone == 1 && g_allocs == 0);
    g_setup_fails = false;
    assert(st.ensure_init() == HC_PHMM_OK && st.stream && st.ready && g_table && g_streams_made == 2);
    assert(st.ensure_init(3) == HC_PHMM_OK && g_streams_made == 2);   // once only
    // buffers grow, release_all drops them and the stream; the next init makes them again
    assert(reserve(b1, 1000, "b1") == 0 && reserve(b2, 10, "b2") == 0 && reserve(b3, 5, "b3") == 0);
    assert(nostream.ensure_init() == HC_PHMM_OK && !nostream.stream && nostream.ready);
    release_all();
    assert(!st.stream && !st.ready && !g_table && !b1.p && !b2.p && !b3.p && b1.bytes == 0 && g_allocs == 0);
    assert(g_streams_gone == 2 && !nostream.ready);
    release_all();   // twice is harmless
    assert(st.ensure_init() == HC_PHMM_OK && g_streams_made == 3);
    // call_frame
    Res* out = reinterpret_cast<Res*>(1);
    assert((call_frame<Res>(nullptr, &st.stream, [](Res&) { return 0; }) == HC_PHMM_EINVAL) && g_err == "null out");
    assert(call_frame(&out, &st.stream, [](Res& r) { r.v.assign(100, 7); return int(HC_PHMM_EHIP); }) == HC_PHMM_EHIP && !out);
    assert(call_frame(&out, &st.stream, [](Res& r) { r.v.assign(100, 7); return 0; }) == HC_PHMM_OK && out && out->v[99] == 7);
    delete out;
    const int syncs = g_syncs;
    assert(call_frame(&out, &st.stream, [](Res&) -> int { throw std::bad_alloc(); }) == HC_PHMM_ENOMEM && !out);
    assert(g_syncs == syncs + 1 && g_err == "host allocation failed");
    assert(call_frame(&out, nullptr, [](Res&) -> int { throw std::bad_alloc(); }) == HC_PHMM_ENOMEM && g_syncs == syncs + 1);
    st.with({&b3});
    assert(reserve(b3, 5, "b3") == 0);
    release_all();
    assert(g_allocs == 0 && g_streams_made == g_streams_gone);
    std::puts("ok");
    return 0;
}
