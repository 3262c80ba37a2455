// Stand-in for kns_engine.cpp in the sanitizer builds of the C-ABI shim (tests/sanitized_build.py, build_abi_driver; SURVEY.md section 5:
// "ASan/UBSan build of the shim").  Only koala_amd/csrc/pv_api*.cpp is under test here -- argument checks, the thread-local error stack,
// string and list ownership -- so the engine behind it is a host-only double: parameters "load" when the file exists, a handle is a plain
// object, process() and run_packets() copy their input, an enable_* call remembers its argument where the inline getters look for it, and no
// HIP call reaches a GPU.  It defines every out-of-line public member of kns::Engine: a new one gets a trivial body here, the engine's
// interface and the product's source files are not shaped around this file.  TEST INFRASTRUCTURE: never linked into the product.
#include <stdio.h>
#include <string.h>

#include "kns_engine.h"

int g_packet_calls = 0;  // run_packets calls that reached the engine

namespace kns {

LoadResult load_params(const char *path, Params *, std::string *err) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        *err = std::string("Failed to open file `") + path + "`.";
        return kLoadIo;
    }
    char magic[8] = {0};
    const size_t n = fread(magic, 1, 8, f);
    fclose(f);
    if (n != 8 || memcmp(magic, "KNS1\0\0\0\0", 8) != 0) {
        *err = std::string("`") + path + "` is not a Koala (KNS1) model file.";
        return kLoadFormat;
    }
    return kLoadOk;
}

static int g_gpus = 1;  // STUB_GPUS=0 in the environment: "no GPU visible"
int visible_gpu_count() {
    const char *e = getenv("STUB_GPUS");
    return e ? atoi(e) : g_gpus;
}
std::string gpu_name(int) { return "Stub GPU"; }

Engine *Engine::create(const Params &, int device, int num_streams, int max_frames, int precision, std::string *err, bool *oom) {
    *oom = false;
    if (getenv("STUB_OOM")) {
        *oom = true;
        *err = "Failed to allocate device memory.";
        return nullptr;
    }
    Engine *e = new Engine();
    e->device_ = device;
    e->B_ = num_streams;
    e->Tmax_ = max_frames;
    e->prec_ = precision;
    if (const char *taps = getenv("STUB_FRONT_TAPS")) e->taps_ = atoi(taps);  // (a model with a several-frame front-end)
    return e;
}
Engine::~Engine() {}
static bool stub_fails(std::string *err) {
    if (getenv("STUB_FAIL_PROCESS")) {
        *err = "HIP error: stub";
        return true;
    }
    if (getenv("STUB_THROW")) throw std::bad_alloc();
    return false;
}
// a stream list as the engine checks it: an index outside the handle is a refused argument, not a failure
static bool stub_list_ok(int count, const int32_t *streams, int B, std::string *err) {
    for (int i = 0; streams && i < count; ++i)
        if (streams[i] < 0 || streams[i] >= B) {
            *err = "`streams[" + std::to_string(i) + "]` is outside the handle.";
            return false;
        }
    return true;
}
Status Engine::process(const Call &c, std::string *err) {
    if (stub_fails(err)) return Status::kRuntime;
    // (every mask is read to its end, as the engine does: a short buffer is the sanitizer's to find)
    unsigned marks = 0;
    for (size_t i = 0; c.resets && i < (size_t) B_ * c.T; ++i) marks += c.resets[i];
    for (int b = 0; c.hold && b < B_; ++b) marks += c.hold[b];
    (void) marks;
    memmove(c.out, c.pcm, (size_t) B_ * c.T * kFrame * 2);
    return Status::kOk;
}
Status Engine::process_host_async(const Call &c, std::string *err) { return process(c, err); }
Status Engine::export_state(int count, const int32_t *streams, void *host_records, std::string *err) {
    if (stub_fails(err)) return Status::kRuntime;
    if (!stub_list_ok(count, streams, B_, err)) return Status::kBadArgument;
    memset(host_records, 0, (size_t) count * state_bytes());
    return Status::kOk;
}
Status Engine::import_state(int count, const int32_t *streams, const void *host_records, std::string *err) {
    if (stub_fails(err)) return Status::kRuntime;
    if (!stub_list_ok(count, streams, B_, err)) return Status::kBadArgument;
    unsigned sum = 0;
    for (size_t i = 0; i < (size_t) count * state_bytes(); ++i) sum += ((const uint8_t *) host_records)[i];
    (void) sum;
    return Status::kOk;
}
// STUB_FAIL_ENABLE=1: the four enable members below fail with a message; STUB_FAIL_ENABLE=throw: they throw as a host allocation would
static bool stub_enables(std::string *err) {
    const char *e = getenv("STUB_FAIL_ENABLE");
    if (e && !strcmp(e, "throw")) throw std::bad_alloc();
    if (e) *err = "Failed to allocate device memory (stub).";
    return !e;
}
bool Engine::enable_packets(int max_samples, std::string *err) {
    if (!stub_enables(err)) return false;
    pk_max_ = max_samples;
    return true;
}
bool Engine::enable_fractional(int rate, int max_samples, std::string *err) {
    if (!stub_enables(err)) return false;
    fr_rate_ = rate, fr_max_ = max_samples;
    return true;
}
bool Engine::set_format(int fmt, std::string *err) {
    if (!stub_enables(err)) return false;
    fmt_ = fmt;
    return true;
}
bool Engine::enable_channels(int C, std::string *err) {
    if (!stub_enables(err)) return false;
    ch_ = C;
    return true;
}
// every stream's counted samples, in elements of the handle's format
Status Engine::run_packets(const PacketCall &c, std::string *) {
    ++g_packet_calls;
    const size_t eb = (size_t) sample_bytes();
    for (int b = 0; b < B_; ++b)
        memmove((uint8_t *) c.out + (size_t) b * c.max_samples * eb, (const uint8_t *) c.pcm + (size_t) b * c.max_samples * eb, (size_t) c.counts[b] * eb);
    return Status::kOk;
}
bool Engine::drain_async(std::string *) { return true; }
bool Engine::async_wait(int, std::string *) { return true; }
bool Engine::reset(const uint8_t *, std::string *) { return true; }
bool Engine::synchronize(std::string *) { return true; }
void Engine::set_stream(hipStream_t s) { stream_ = s ? s : own_stream_; }
void Engine::profile_enable(bool on) { profiling_ = on; }
bool Engine::profile_read(double *ms, int64_t *launches, std::string *) {
    for (int i = 0; i < kNumKernelClasses; ++i) ms[i] = 0.0, launches[i] = 0;
    return true;
}
int64_t Engine::debug_read(int, float *, int64_t, std::string *err) {
    *err = "unknown debug tap";
    return -1;
}

}  // namespace kns

// the three HIP entry points pv_api.cpp calls directly (page-locked buffers): host memory, no runtime
extern "C" {
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) {
    *ptr = malloc(size);
    return *ptr ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void *ptr) {
    free(ptr);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}
