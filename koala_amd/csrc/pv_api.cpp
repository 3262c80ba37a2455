// pv_api.cpp -- the C ABI of libpv_koala.so: single-stream entry points of include/pv_koala.h + include/picovoice.h
// and the batch extension of include/pv_koala_batch.h, all driving kns::Engine (HIP, gfx950).
//
// Behaviour at the boundary follows what the reference library was observed to do:
// argument checks in the same order (NULL arguments -> model file -> device string -> device availability),
// the same status codes and message texts, a thread-local error stack of at most 8 messages drained by one
// pv_get_error_stack call, pv_koala_delete(NULL) a no-op.  There is no CPU compute path in this library: a call
// that needs the GPU and cannot reach one fails with a status and a message, it never falls back.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pv_koala.h"
#include "../../include/pv_koala_batch.h"
#include "kns_engine.h"
#include "pv_api_internal.h"

#ifdef KNS_TIMING
namespace kns {
void read_timing(unsigned long long *out);
}
#endif

namespace {

using kns_api::guarded;

const char kBuildId[] = "a355c0a";  // 7 hex digits, as the reference prints in front of every message

// the calling thread's error stack (at most 8 messages, drained by pv_get_error_stack): every entry point clears it first
thread_local std::vector<std::string> t_stack;

void push_error(unsigned code, const char *fmt, ...) {
    char text[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
    char line[832];
    snprintf(line, sizeof(line), "%s %08X: %s", kBuildId, code, text);
    if (t_stack.size() < 8) t_stack.push_back(line);
}

// ---- the argument checks that several entry points share: the first failure's message and status, in this order
pv_status_t check_object(const void *object) {
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return PV_STATUS_SUCCESS;
}

pv_status_t check_call(const pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm, const int16_t *enhanced) {
    if (!object) return check_object(object);
    if (object->packet_samples) {  // every frame entry point comes through here
        push_error(0x66, "Frame calls are not available on a packet handle: its streams advance through pv_koala_batch_process_packets.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!pcm || !enhanced) {
        push_error(0x64, "Argument `%s` is NULL.", pcm ? "enhanced" : "pcm");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (num_frames <= 0 || num_frames > object->engine->max_frames()) {
        push_error(0x66, "`num_frames` %d is outside [1, %d].", num_frames, object->engine->max_frames());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return PV_STATUS_SUCCESS;
}

// handles that are not at 16 kHz, handles with a sample format and handles with channels have no asynchronous path yet
pv_status_t check_synchronous(const pv_koala_batch_t *object) {
    if (object->engine->channels() != 1) {
        push_error(0x66, "Asynchronous calls are not available on a handle whose `channels` is %d, not 1.", object->engine->channels());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (object->sample_rate != kns::kRate16k) {
        push_error(0x66, "Asynchronous calls are not available on a handle whose sample rate is %d, not 16000.", object->sample_rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (object->engine->sample_format() != kns::kFmtS16) {
        push_error(0x66, "Asynchronous calls are not available on a handle whose sample format is %d, not PV_KOALA_SAMPLE_S16.",
                   object->engine->sample_format());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return PV_STATUS_SUCCESS;
}

// the five-frame front-end takes per-frame stream resets at frame 0 only (the reset kernel)
pv_status_t check_resets(const pv_koala_batch_t *object, int32_t num_frames, const uint8_t *reset) {
    if (!reset || object->engine->front_taps() <= 1) return PV_STATUS_SUCCESS;
    const int32_t B = object->engine->num_streams();
    for (int32_t b = 0; b < B; ++b)
        for (int32_t t = 1; t < num_frames; ++t)
            if (reset[(size_t) b * num_frames + t]) {
                push_error(0x66, "`reset[%d][%d]` is set: a model with a %d-frame front-end takes per-frame stream resets at frame 0 only.",
                           b, t, object->engine->front_taps());
                return PV_STATUS_INVALID_ARGUMENT;
            }
    return PV_STATUS_SUCCESS;
}

// a handle at 44 100 or 22 050 Hz (pv_api_extensions.cpp) has no stream records yet, and no whole frame
pv_status_t check_records(const pv_koala_batch_t *object) {
    if (kns::fr_rate_ok(object->sample_rate)) {
        push_error(0x66, "Stream records (state_size, export_state, import_state) are not available yet on a handle whose sample rate is %d.",
                   object->sample_rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (object->settings.high_band) {  // (a record would need the feature's per-stream state)
        push_error(0x66, "Stream records (state_size, export_state, import_state) are not available yet while the high-band carry is on "
                         "(pv_koala_batch_set_high_band).");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return PV_STATUS_SUCCESS;
}

pv_status_t check_list(const pv_koala_batch_t *object, int32_t count, const void *records) {
    if (!object) return check_object(object);
    if (check_records(object) != PV_STATUS_SUCCESS) return PV_STATUS_INVALID_ARGUMENT;
    if (!records) {
        push_error(0x64, "Argument `records` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (count < 1 || count > object->engine->num_streams()) {
        push_error(0x66, "`count` %d is outside [1, %d].", count, object->engine->num_streams());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return PV_STATUS_SUCCESS;
}

// what an engine call that did not succeed leaves on the stack: a refused argument, or a failure under the entry point's own code
pv_status_t engine_failure(kns::Status status, unsigned runtime_code, const std::string &err) {
    if (status == kns::Status::kBadArgument) {
        push_error(0x66, "%s", err.c_str());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    push_error(runtime_code, "%s", err.c_str());
    push_error(0x12C, "Picovoice Error.");
    return PV_STATUS_RUNTIME_ERROR;
}

// one call that advances the streams (arguments already checked), under the handle's settings
pv_status_t advance(kns::Engine *engine, const HandleSettings &settings, kns::Call call, bool async = false) {
    if (kns_api::check_settings(settings, engine, async) != PV_STATUS_SUCCESS) return PV_STATUS_INVALID_ARGUMENT;
    kns_api::carry(settings, &call.opt);
    if (settings.high_band) {  // what the high-band carry does not take yet: refused here, before the engine is reached
        const int32_t B = engine->num_streams();
        for (int32_t b = 0; call.hold && b < B; ++b)
            if (call.hold[b]) {
                push_error(0x66, "`hold[%d]` is set: `hold` is not available yet while the high-band carry is on (pv_koala_batch_set_high_band).", b);
                return PV_STATUS_INVALID_ARGUMENT;
            }
        for (int32_t b = 0; call.resets && b < B; ++b)
            for (int32_t t = 1; t < call.T; ++t)
                if (call.resets[(size_t) b * call.T + t]) {
                    push_error(0x66, "`reset[%d][%d]` is set: while the high-band carry is on (pv_koala_batch_set_high_band) a handle takes "
                                     "per-frame stream resets at frame 0 only (not yet).", b, t);
                    return PV_STATUS_INVALID_ARGUMENT;
                }
        call.high_band = settings.high_band, call.high_band_epoch = settings.high_band_epoch;
    }
    return guarded([&] {
        std::string err;
        const kns::Status status = async ? engine->process_host_async(call, &err) : engine->process(call, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : engine_failure(status, async ? 0x33A : 0x337, err);
    });
}

}  // namespace

// what the other translation unit of the C ABI (pv_api_extensions.cpp) shares with this one: pv_api_internal.h
namespace kns_api {
void clear_errors() { t_stack.clear(); }
void push_error(unsigned code, const char *fmt, ...) {
    char text[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
    ::push_error(code, "%s", text);
}
pv_status_t engine_failure(kns::Status status, unsigned runtime_code, const std::string &err) { return ::engine_failure(status, runtime_code, err); }
// an output stage that is on: `stage`, `setter`: what the message calls it; `link`, `high_band`: why not with the link / the carry
static pv_status_t check_stage(bool on, const char *stage, const char *setter, const char *link, const char *high_band, const HandleSettings &s,
                               const kns::Engine *engine, bool async) {
    if (!on) return PV_STATUS_SUCCESS;
    const char *what = s.link                  ? "while the channel link is on (pv_koala_batch_set_channel_link): " :
                       s.high_band             ? "while the high-band carry is on (pv_koala_batch_set_high_band): " :
                       async                   ? "on the asynchronous entry points" :
                       engine->fractional_rate() ? "on a handle whose sample rate is 44100 or 22050" : nullptr;
    if (!what) return PV_STATUS_SUCCESS;
    ::push_error(0x66, "%s (%s: some stream's `on` is set) is not available yet %s%s.", stage, setter, what, s.link ? link : s.high_band ? high_band : "");
    return PV_STATUS_INVALID_ARGUMENT;
}
pv_status_t check_settings(const HandleSettings &s, const kns::Engine *engine, bool async) {
    if (s.profile_any && s.link) {
        ::push_error(0x66, "A band profile that is not neutral (pv_koala_batch_set_band_profile) is not available yet while the channel link is on "
                           "(pv_koala_batch_set_channel_link).");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (s.profile_any && s.high_band) {
        ::push_error(0x66, "A band profile that is not neutral (pv_koala_batch_set_band_profile) is not available yet while the high-band carry is on "
                           "(pv_koala_batch_set_high_band): its broadband gain would have to follow the profile.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const char *one_gain = "a group would need one gain", *same_gain = "its band would need the same gain";
    if (check_stage(s.level_any, "The output leveller", "pv_koala_batch_set_level", one_gain, same_gain, s, engine, async) != PV_STATUS_SUCCESS ||
        check_stage(s.limiter_any, "The peak limiter", "pv_koala_batch_set_limiter", one_gain, same_gain, s, engine, async) != PV_STATUS_SUCCESS ||
        check_stage(s.comfort_any, "Comfort noise", "pv_koala_batch_set_comfort_noise", "a group would need one fill",
                    "its broadband gain would have to see the fill", s, engine, async) != PV_STATUS_SUCCESS)
        return PV_STATUS_INVALID_ARGUMENT;
    return PV_STATUS_SUCCESS;
}
}  // namespace kns_api

namespace {

std::mutex g_sdk_mutex;
std::string g_sdk = "c";
bool g_log = false;

const char *const kStatusNames[] = {"SUCCESS",          "OUT_OF_MEMORY",           "IO_ERROR",
                                    "INVALID_ARGUMENT", "STOP_ITERATION",          "KEY_ERROR",
                                    "INVALID_STATE",    "RUNTIME_ERROR",           "ACTIVATION_ERROR",
                                    "ACTIVATION_LIMIT_REACHED", "ACTIVATION_THROTTLED", "ACTIVATION_REFUSED"};

enum DeviceKind { kDevBest, kDevCpu, kDevGpu };
struct DeviceSpec {
    DeviceKind kind;
    int index;  // gpu index or cpu thread count; -1 = unspecified
};

// grammar of the reference's `device` argument (include/pv_koala.h:42-46): best | cpu | cpu:N | gpu | gpu:N
bool parse_device(const char *text, DeviceSpec *out) {
    // an entry of pv_koala_list_hardware_devices ("gpu:0 - <name>") is accepted as it was printed
    std::string head(text);
    const size_t dash = head.find(" - ");
    if (dash != std::string::npos && dash > 0) head.resize(dash);
    const char *s = head.c_str();
    auto number = [](const char *p, int *v) {
        if (!*p) return false;
        long n = 0;
        for (; *p; ++p) {
            if (*p < '0' || *p > '9') return false;
            n = n * 10 + (*p - '0');
            if (n > 1 << 20) return false;
        }
        *v = (int) n;
        return true;
    };
    if (!strcmp(s, "best")) {
        *out = {kDevBest, -1};
        return true;
    }
    if (!strcmp(s, "cpu")) {
        *out = {kDevCpu, -1};
        return true;
    }
    if (!strcmp(s, "gpu")) {
        *out = {kDevGpu, -1};
        return true;
    }
    int v;
    if (!strncmp(s, "cpu:", 4) && number(s + 4, &v)) {
        *out = {kDevCpu, v};
        return true;
    }
    if (!strncmp(s, "gpu:", 4) && number(s + 4, &v)) {
        *out = {kDevGpu, v};
        return true;
    }
    return false;
}

// shared front half of pv_koala_init / pv_koala_batch_init
pv_status_t open_engine_unguarded(const char *access_key, const char *model_path, const char *device, void *object,
                                  int num_streams, int max_frames, int precision, int sample_rate, kns::Engine **engine) {
    if (!access_key) {
        push_error(0x64, "Argument `access_key` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!model_path) {
        push_error(0x64, "Argument `model_path` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!device) {  // the reference dereferences NULL here; an argument error is the drop-in-safe behaviour
        push_error(0x64, "Argument `device` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!object) return check_object(object);
    kns::Params params;
    std::string err;
    kns::LoadResult lr = kns::load_params(model_path, &params, &err);
    if (lr == kns::kLoadIo) {
        push_error(0xC9, "%s", err.c_str());
        push_error(0x136, "Koala model (.kns) could not be opened.");
        return PV_STATUS_IO_ERROR;
    }
    if (lr != kns::kLoadOk) {
        push_error(0xCA, "%s", err.c_str());
        push_error(0x136, "Koala model (.kns) could not be read.");
        return PV_STATUS_IO_ERROR;
    }
    DeviceSpec spec;
    if (!parse_device(device, &spec)) {
        push_error(0x322, "%s is not a valid device string", device);
        push_error(0x12C, "Picovoice Error.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (spec.kind == kDevCpu) {
        push_error(0x323, "Device `%s` is not available: this build has no CPU backend, use `best`, `gpu` or `gpu:N`.",
                   device);
        push_error(0x12C, "Picovoice Error.");
        return PV_STATUS_RUNTIME_ERROR;
    }
    const int ngpu = kns::visible_gpu_count();
    if (ngpu <= 0) {
        push_error(0x334, "Failed to communicate with device.");
        push_error(0x12C, "Picovoice Error.");
        return PV_STATUS_RUNTIME_ERROR;
    }
    const int index = spec.index < 0 ? 0 : spec.index;
    if (index >= ngpu) {
        push_error(0x335, "GPU device index `%d` is out of range. %d device(s) available.", index, ngpu);
        push_error(0x12C, "Picovoice Error.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!*access_key) {
        push_error(0x190, "Failed to parse AccessKey ``.");
        push_error(0x12C, "Picovoice Error.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    params.sample_rate = sample_rate;
    bool oom = false;
    kns::Engine *e = kns::Engine::create(params, index, num_streams, max_frames, precision, &err, &oom);
    if (!e) {
        push_error(oom ? 0x65 : 0x336, "%s", err.c_str());
        push_error(0x12C, "Picovoice Error.");
        return oom ? PV_STATUS_OUT_OF_MEMORY : PV_STATUS_RUNTIME_ERROR;
    }
    *engine = e;
    return PV_STATUS_SUCCESS;
}

pv_status_t open_engine(const char *access_key, const char *model_path, const char *device, void *object, int num_streams,
                        int max_frames, int precision, int sample_rate, kns::Engine **engine) {
    return guarded([&] {
        return open_engine_unguarded(access_key, model_path, device, object, num_streams, max_frames, precision, sample_rate, engine);
    });
}

// the handle around a new engine (takes the engine over: deleted when the handle cannot be made)
template <class H>
pv_status_t make_handle(kns::Engine *e, H **object) {
    H *o = nullptr;
    try {
        o = new H();
        o->engine = e;
        o->settings.gain.assign((size_t) e->num_streams(), 0.0f);
    } catch (...) {
        delete o;
        o = nullptr;
    }
    if (!o) {
        delete e;
        push_error(0x65, "Failed to allocate memory.");
        return PV_STATUS_OUT_OF_MEMORY;
    }
    *object = o;
    return PV_STATUS_SUCCESS;
}

// pv_koala_batch_set_min_gain / pv_koala_set_min_gain: every entry is checked before anything is changed
pv_status_t set_min_gain(HandleSettings *settings, int32_t B, int32_t count, const int32_t *streams, const float *gains) {
    if (!gains) {
        push_error(0x64, "Argument `gains` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (count < 1 || count > B) {
        push_error(0x66, "`count` %d is outside [1, %d].", count, B);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return guarded([&] {
        std::vector<float> next(settings->gain);
        std::vector<uint8_t> listed((size_t) B, 0);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t b = kns_api::listed_stream(&listed, streams, i);
            if (b < 0) return PV_STATUS_INVALID_ARGUMENT;
            if (!(gains[i] >= 0.0f && gains[i] <= 1.0f)) {  // (NaN fails both comparisons)
                push_error(0x66, "gain %d: %g is not a minimum gain in [0, 1].", i, (double) gains[i]);
                return PV_STATUS_INVALID_ARGUMENT;
            }
            next[b] = gains[i] + 0.0f;  // (-0 -> +0: "no limit" is one bit pattern)
        }
        bool any = false;
        for (float g : next) any = any || g != 0.0f;
        settings->gain.swap(next);
        settings->any = any;
        ++settings->rev;
        return PV_STATUS_SUCCESS;
    });
}

// pv_koala_batch_set_band_profile / pv_koala_set_band_profile: every value is checked before anything is changed
pv_status_t set_band_profile(HandleSettings *settings, int32_t B, int32_t count, const int32_t *streams, const float *floor, const float *ceil) {
    if (count < 1 || count > B) {
        push_error(0x66, "`count` %d is outside [1, %d].", count, B);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return guarded([&] {
        constexpr int K = PV_KOALA_NUM_BINS, R = kns::kProfileRow;
        std::vector<float> next(settings->profile);
        if (next.empty()) {  // the neutral table
            next.assign((size_t) B * R, 0.0f);
            for (int32_t b = 0; b < B; ++b)
                for (int k = 0; k < K; ++k) next[(size_t) b * R + kns::profile_index(k, 1)] = 1.0f;
        }
        std::vector<uint8_t> listed((size_t) B, 0);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t b = kns_api::listed_stream(&listed, streams, i);
            if (b < 0) return PV_STATUS_INVALID_ARGUMENT;
            for (int k = 0; k < K; ++k) {
                const float lo = floor ? floor[(size_t) i * K + k] : 0.0f, hi = ceil ? ceil[(size_t) i * K + k] : 1.0f;
                if (!(lo >= 0.0f && lo <= 1.0f) || !(hi >= 0.0f && hi <= 1.0f)) {  // (NaN fails both comparisons)
                    const bool is_floor = !(lo >= 0.0f && lo <= 1.0f);
                    push_error(0x66, "profile %d, bin %d: %s %g is not in [0, 1].", i, k, is_floor ? "floor" : "ceiling", (double) (is_floor ? lo : hi));
                    return PV_STATUS_INVALID_ARGUMENT;
                }
                if (lo > hi) {
                    push_error(0x66, "profile %d, bin %d: floor %g is above ceiling %g.", i, k, (double) lo, (double) hi);
                    return PV_STATUS_INVALID_ARGUMENT;
                }
                next[(size_t) b * R + kns::profile_index(k, 0)] = lo + 0.0f;  // (-0 -> +0: the kernel orders the bit patterns)
                next[(size_t) b * R + kns::profile_index(k, 1)] = hi + 0.0f;
            }
        }
        bool any = false;
        for (int32_t b = 0; b < B && !any; ++b)
            for (int k = 0; k < K && !any; ++k)
                any = next[(size_t) b * R + kns::profile_index(k, 0)] != 0.0f || next[(size_t) b * R + kns::profile_index(k, 1)] != 1.0f;
        settings->profile.swap(next);
        settings->profile_any = any;
        ++settings->profile_rev;
        return PV_STATUS_SUCCESS;
    });
}

void get_band_profile(const HandleSettings &settings, int32_t b, float *floor, float *ceil) {
    for (int k = 0; k < PV_KOALA_NUM_BINS; ++k) {
        const bool set = !settings.profile.empty();
        if (floor) floor[k] = set ? settings.profile[(size_t) b * kns::kProfileRow + kns::profile_index(k, 0)] : 0.0f;
        if (ceil) ceil[k] = set ? settings.profile[(size_t) b * kns::kProfileRow + kns::profile_index(k, 1)] : 1.0f;
    }
}

int default_precision() {
    const char *p = getenv("KOALA_AMD_PRECISION");
    if (p && !strcmp(p, "bf16")) return kns::kBf16;
    return kns::kFp32;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------ picovoice.h

PV_API int32_t pv_sample_rate(void) { return 16000; }

PV_API const char *pv_status_to_string(pv_status_t status) {
    if ((int) status < 0 || (int) status > 11) return NULL;
    return kStatusNames[(int) status];
}

PV_API pv_status_t pv_get_error_stack(char ***message_stack, int32_t *message_stack_depth) {
    if (!message_stack || !message_stack_depth) return PV_STATUS_INVALID_ARGUMENT;
    const size_t n = t_stack.size();
    if (n == 0) {  // nothing pending: no allocation either -- a caller that sees a failure status frees nothing (found by the ASan build)
        *message_stack = NULL;
        *message_stack_depth = 0;
        return PV_STATUS_INVALID_STATE;
    }
    char **arr = (char **) calloc(n + 1, sizeof(char *));
    if (!arr) return PV_STATUS_OUT_OF_MEMORY;
    for (size_t i = 0; i < n; ++i) arr[i] = strdup(t_stack[i].c_str());
    t_stack.clear();
    *message_stack = arr;
    *message_stack_depth = (int32_t) n;
    return PV_STATUS_SUCCESS;
}

PV_API void pv_free_error_stack(char **message_stack) {
    if (!message_stack) return;
    for (char **p = message_stack; *p; ++p) free(*p);
    free(message_stack);
}

PV_API void pv_set_sdk(const char *sdk) {
    std::lock_guard<std::mutex> lock(g_sdk_mutex);
    if (sdk) g_sdk = sdk;
}

PV_API const char *pv_get_sdk(void) {
    std::lock_guard<std::mutex> lock(g_sdk_mutex);
    static thread_local std::string copy;
    copy = g_sdk;
    return copy.c_str();
}

PV_API void pv_free(void *ptr) { free(ptr); }
PV_API void pv_log_enable(void) { g_log = true; }
PV_API void pv_log_disable(void) { g_log = false; }

// ------------------------------------------------------------------------------------------------ pv_koala.h

PV_API pv_status_t pv_koala_init(const char *access_key, const char *model_path, const char *device,
                                 pv_koala_t **object) {
    t_stack.clear();
    kns::Engine *e = nullptr;
    pv_status_t st = open_engine(access_key, model_path, device, object, 1, 1, default_precision(), kns::kRate16k, &e);
    if (st != PV_STATUS_SUCCESS) return st;
    return make_handle(e, object);
}

PV_API void pv_koala_delete(pv_koala_t *object) {
    if (!object) return;
    delete object->engine;
    delete object;
}

PV_API pv_status_t pv_koala_process(pv_koala_t *object, const int16_t *pcm, int16_t *enhanced_pcm) {
    t_stack.clear();
    if (!object) return check_object(object);
    if (!pcm) {
        push_error(0x64, "Argument `pcm` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!enhanced_pcm) {
        push_error(0x64, "Argument `enhanced_pcm` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return advance(object->engine, object->settings, {1, pcm, enhanced_pcm, nullptr, nullptr, /*host_contract=*/true});
}

PV_API pv_status_t pv_koala_process_report(pv_koala_t *object, const int16_t *pcm, int16_t *enhanced_pcm, float report[4]) {
    t_stack.clear();
    if (!object) return check_object(object);
    if (!pcm || !enhanced_pcm || !report) {
        push_error(0x64, "Argument `%s` is NULL.", !pcm ? "pcm" : !enhanced_pcm ? "enhanced_pcm" : "report");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    kns::Call call{1, pcm, enhanced_pcm, nullptr, nullptr, /*host_contract=*/true};
    call.report = report;
    return advance(object->engine, object->settings, call);
}

PV_API pv_status_t pv_koala_reset(pv_koala_t *object) {
    t_stack.clear();
    if (!object) return PV_STATUS_INVALID_ARGUMENT;  // the reference leaves no message for this one
    return guarded([&] {
        std::string err;
        if (!object->engine->reset(nullptr, &err)) {
            push_error(0x338, "%s", err.c_str());
            return PV_STATUS_RUNTIME_ERROR;
        }
        return PV_STATUS_SUCCESS;
    });
}

PV_API pv_status_t pv_koala_delay_sample(const pv_koala_t *object, int32_t *delay_sample) {
    t_stack.clear();
    if (!object) return check_object(object);
    if (!delay_sample) {
        push_error(0x64, "Argument `delay_sample` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *delay_sample = kns::kFrame;
    return PV_STATUS_SUCCESS;
}

PV_API int32_t pv_koala_frame_length(void) { return kns::kFrame; }

PV_API const char *pv_koala_version(void) { return "3.0.0"; }

PV_API pv_status_t pv_koala_list_hardware_devices(char ***hardware_devices, int32_t *num_hardware_devices) {
    if (!hardware_devices || !num_hardware_devices) return PV_STATUS_INVALID_ARGUMENT;
    const int n = kns::visible_gpu_count();
    char **arr = (char **) calloc((size_t) n + 1, sizeof(char *));
    if (!arr) return PV_STATUS_OUT_OF_MEMORY;
    for (int i = 0; i < n; ++i) {
        char line[320];
        snprintf(line, sizeof(line), "gpu:%d - %s", i, kns::gpu_name(i).c_str());
        arr[i] = strdup(line);
    }
    *hardware_devices = arr;
    *num_hardware_devices = n;
    return PV_STATUS_SUCCESS;
}

PV_API void pv_koala_free_hardware_devices(char **hardware_devices, int32_t num_hardware_devices) {
    if (!hardware_devices) return;
    for (int32_t i = 0; i < num_hardware_devices; ++i) free(hardware_devices[i]);
    free(hardware_devices);
}

// ------------------------------------------------------------------------------------------------ pv_koala_batch.h

PV_API pv_status_t pv_koala_batch_init(const char *access_key, const char *model_path, const char *device,
                                       int32_t num_streams, int32_t max_frames_per_call,
                                       pv_koala_precision_t precision, pv_koala_batch_t **object) {
    return pv_koala_batch_init_rate(access_key, model_path, device, num_streams, max_frames_per_call, precision, kns::kRate16k, object);
}

PV_API pv_status_t pv_koala_batch_init_rate(const char *access_key, const char *model_path, const char *device,
                                            int32_t num_streams, int32_t max_frames_per_call,
                                            pv_koala_precision_t precision, int32_t sample_rate, pv_koala_batch_t **object) {
    t_stack.clear();
    if (num_streams <= 0 || max_frames_per_call <= 0) {
        push_error(0x66, "`num_streams` and `max_frames_per_call` must be positive.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (precision != PV_KOALA_PRECISION_FP32 && precision != PV_KOALA_PRECISION_BF16) {
        push_error(0x66, "`precision` must be PV_KOALA_PRECISION_FP32 or PV_KOALA_PRECISION_BF16.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!kns::rs_rate_ok(sample_rate)) {
        push_error(0x66, "`sample_rate` %d is not one of 8000, 12000, 16000, 24000, 32000, 48000.", sample_rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    kns::Engine *e = nullptr;
    pv_status_t st = open_engine(access_key, model_path, device, object, num_streams, max_frames_per_call,
                                 precision == PV_KOALA_PRECISION_BF16 ? kns::kBf16 : kns::kFp32, sample_rate, &e);
    if (st != PV_STATUS_SUCCESS) return st;
    st = make_handle(e, object);
    if (st == PV_STATUS_SUCCESS) (*object)->sample_rate = sample_rate;
    return st;
}

PV_API void pv_koala_batch_delete(pv_koala_batch_t *object) {
    if (!object) return;
    delete object->engine;
    delete object;
}

PV_API pv_status_t pv_koala_batch_process_chunk(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                int16_t *enhanced) {
    t_stack.clear();
    const pv_status_t st = check_call(object, num_frames, pcm, enhanced);
    if (st != PV_STATUS_SUCCESS) return st;
    return advance(object->engine, object->settings, {num_frames, pcm, enhanced});
}

PV_API pv_status_t pv_koala_batch_process_chunk_async(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                      int16_t *enhanced) {
    t_stack.clear();
    pv_status_t st = check_call(object, num_frames, pcm, enhanced);
    if (st == PV_STATUS_SUCCESS) st = check_synchronous(object);
    if (st != PV_STATUS_SUCCESS) return st;
    return advance(object->engine, object->settings, {num_frames, pcm, enhanced}, /*async=*/true);
}

PV_API pv_status_t pv_koala_batch_process_chunk_resets(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                       int16_t *enhanced, const uint8_t *reset) {
    t_stack.clear();
    pv_status_t st = check_call(object, num_frames, pcm, enhanced);
    if (st == PV_STATUS_SUCCESS) st = check_resets(object, num_frames, reset);
    if (st != PV_STATUS_SUCCESS) return st;
    return advance(object->engine, object->settings, {num_frames, pcm, enhanced, reset});
}

PV_API pv_status_t pv_koala_batch_process_chunk_resets_async(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                             int16_t *enhanced, const uint8_t *reset) {
    t_stack.clear();
    pv_status_t st = check_call(object, num_frames, pcm, enhanced);
    if (st == PV_STATUS_SUCCESS) st = check_resets(object, num_frames, reset);
    if (st == PV_STATUS_SUCCESS) st = check_synchronous(object);
    if (st != PV_STATUS_SUCCESS) return st;
    return advance(object->engine, object->settings, {num_frames, pcm, enhanced, reset}, /*async=*/true);
}

PV_API pv_status_t pv_koala_batch_process_chunk_hold(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                     int16_t *enhanced, const uint8_t *hold) {
    t_stack.clear();
    const pv_status_t st = check_call(object, num_frames, pcm, enhanced);
    if (st != PV_STATUS_SUCCESS) return st;
    return advance(object->engine, object->settings, {num_frames, pcm, enhanced, nullptr, hold});
}

// ---- one extensible entry point (the frame report rides on it)

PV_API pv_status_t pv_koala_batch_process_call(pv_koala_batch_t *object, const pv_koala_batch_call_t *call) {
    t_stack.clear();
    if (!object) return check_object(object);
    if (!call) {
        push_error(0x64, "Argument `call` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (call->struct_size != (int32_t) sizeof(pv_koala_batch_call_t)) {
        push_error(0x66, "`struct_size` %d is not sizeof(pv_koala_batch_call_t) = %d.", call->struct_size, (int) sizeof(pv_koala_batch_call_t));
        return PV_STATUS_INVALID_ARGUMENT;
    }
    pv_status_t st = check_call(object, call->num_frames, call->pcm, call->enhanced);
    if (st == PV_STATUS_SUCCESS) st = check_resets(object, call->num_frames, call->reset);
    if (st == PV_STATUS_SUCCESS && call->asynchronous != 0) st = check_synchronous(object);
    if (st != PV_STATUS_SUCCESS) return st;
    kns::Call c{call->num_frames, call->pcm, call->enhanced, call->reset, call->hold};
    c.report = call->report;
    // (hold with reset, hold with asynchronous: refused by the engine before it touches anything, as for the dedicated entry points)
    return advance(object->engine, object->settings, c, call->asynchronous != 0);
}

// ---- attenuation limit

PV_API pv_status_t pv_koala_batch_set_min_gain(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const float *gains) {
    t_stack.clear();
    if (!object) return check_object(object);
    return set_min_gain(&object->settings, object->engine->num_streams(), count, streams, gains);
}

PV_API pv_status_t pv_koala_batch_get_min_gain(const pv_koala_batch_t *object, float *gains) {
    t_stack.clear();
    if (!object || !gains) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "gains" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    memcpy(gains, object->settings.gain.data(), object->settings.gain.size() * sizeof(float));
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_set_min_gain(pv_koala_t *object, float gain) {
    t_stack.clear();
    if (!object) return check_object(object);
    return set_min_gain(&object->settings, 1, 1, nullptr, &gain);
}

PV_API pv_status_t pv_koala_get_min_gain(const pv_koala_t *object, float *gain) {
    t_stack.clear();
    if (!object || !gain) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "gain" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *gain = object->settings.gain[0];
    return PV_STATUS_SUCCESS;
}

// ---- band profile

PV_API pv_status_t pv_koala_batch_set_band_profile(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const float *floor,
                                                   const float *ceil) {
    t_stack.clear();
    if (!object) return check_object(object);
    return set_band_profile(&object->settings, object->engine->num_streams(), count, streams, floor, ceil);
}

PV_API pv_status_t pv_koala_batch_get_band_profile(const pv_koala_batch_t *object, int32_t stream, float *floor, float *ceil) {
    t_stack.clear();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (stream < 0 || stream >= object->engine->num_streams()) {
        push_error(0x66, "`stream` %d is outside [0, %d).", stream, object->engine->num_streams());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    get_band_profile(object->settings, stream, floor, ceil);
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_set_band_profile(pv_koala_t *object, const float *floor, const float *ceil) {
    t_stack.clear();
    if (!object) return check_object(object);
    return set_band_profile(&object->settings, 1, 1, nullptr, floor, ceil);
}

PV_API pv_status_t pv_koala_get_band_profile(const pv_koala_t *object, float *floor, float *ceil) {
    t_stack.clear();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    get_band_profile(object->settings, 0, floor, ceil);
    return PV_STATUS_SUCCESS;
}

// ---- stream records

PV_API pv_status_t pv_koala_batch_state_size(const pv_koala_batch_t *object, int32_t *num_bytes) {
    t_stack.clear();
    if (!object || !num_bytes) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "num_bytes" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (check_records(object) != PV_STATUS_SUCCESS) return PV_STATUS_INVALID_ARGUMENT;
    *num_bytes = (int32_t) (kns::state_record_bytes(object->engine->front_taps(), object->sample_rate) +
                            (object->packet_samples ? kns::pk_record_bytes(object->sample_rate) : 0));
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_export_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, void *records) {
    t_stack.clear();
    const pv_status_t st = check_list(object, count, records);
    if (st != PV_STATUS_SUCCESS) return st;
    return guarded([&] {
        std::string err;
        const kns::Status status = object->engine->export_state(count, streams, records, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : engine_failure(status, 0x33C, err);
    });
}

PV_API pv_status_t pv_koala_batch_import_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams,
                                               const void *records) {
    t_stack.clear();
    const pv_status_t st = check_list(object, count, records);
    if (st != PV_STATUS_SUCCESS) return st;
    return guarded([&] {
        std::string err;
        const kns::Status status = object->engine->import_state(count, streams, records, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : engine_failure(status, 0x33C, err);
    });
}

PV_API pv_status_t pv_koala_batch_async_wait(pv_koala_batch_t *object, int32_t max_in_flight) {
    t_stack.clear();
    if (!object) return check_object(object);
    if (max_in_flight < 0) {
        push_error(0x66, "`max_in_flight` %d is negative.", max_in_flight);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return guarded([&] {
        std::string err;
        if (!object->engine->async_wait(max_in_flight, &err)) {
            push_error(0x33B, "%s", err.c_str());
            return PV_STATUS_RUNTIME_ERROR;
        }
        return PV_STATUS_SUCCESS;
    });
}

PV_API pv_status_t pv_koala_batch_process(pv_koala_batch_t *object, const int16_t *pcm, int16_t *enhanced) {
    return pv_koala_batch_process_chunk(object, 1, pcm, enhanced);
}

PV_API pv_status_t pv_koala_batch_reset(pv_koala_batch_t *object, const uint8_t *stream_mask) {
    t_stack.clear();
    if (!object) return check_object(object);
    return guarded([&] {
        std::string err;
        if (!object->engine->reset(stream_mask, &err)) {
            push_error(0x338, "%s", err.c_str());
            return PV_STATUS_RUNTIME_ERROR;
        }
        return PV_STATUS_SUCCESS;
    });
}

PV_API pv_status_t pv_koala_batch_num_streams(const pv_koala_batch_t *object, int32_t *num_streams) {
    t_stack.clear();
    if (!object || !num_streams) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "num_streams" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *num_streams = object->engine->num_streams();
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_delay_sample(const pv_koala_batch_t *object, int32_t *delay_sample) {
    t_stack.clear();
    if (!object || !delay_sample) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "delay_sample" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (kns::fr_rate_ok(object->sample_rate)) {  // both fractional stages and the inner packet handle's 511 samples, a whole number by c
        *delay_sample = kns::fr_delay(kns::fr_up(object->sample_rate));
        return PV_STATUS_SUCCESS;
    }
    // (a packet handle: and the F - 1 samples in front of its output stream)
    *delay_sample = kns::rs_frame_length(object->sample_rate) + kns::rs_delay(object->sample_rate) +
                    (object->packet_samples ? kns::rs_frame_length(object->sample_rate) - 1 : 0);
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_sample_rate(const pv_koala_batch_t *object, int32_t *sample_rate) {
    t_stack.clear();
    if (!object || !sample_rate) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "sample_rate" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *sample_rate = object->sample_rate;
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_frame_length(const pv_koala_batch_t *object, int32_t *frame_length) {
    t_stack.clear();
    if (!object || !frame_length) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "frame_length" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (kns::fr_rate_ok(object->sample_rate)) {
        push_error(0x66, "A handle whose sample rate is %d has no frame length: 16 ms is not a whole number of samples there.", object->sample_rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *frame_length = kns::rs_frame_length(object->sample_rate);
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_set_stream(pv_koala_batch_t *object, void *hip_stream) {
    t_stack.clear();
    if (!object) return check_object(object);
    object->engine->set_stream((hipStream_t) hip_stream);
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_host_alloc(int64_t num_bytes, void **memory) {
    t_stack.clear();
    if (!memory) {
        push_error(0x64, "Argument `memory` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *memory = nullptr;
    if (num_bytes <= 0) {
        push_error(0x65, "`num_bytes` should be positive.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (kns::visible_gpu_count() <= 0) {
        push_error(0x33A, "No GPU is visible: page-locked memory needs the HIP runtime.");
        return PV_STATUS_RUNTIME_ERROR;
    }
    if (hipHostMalloc(memory, (size_t) num_bytes, hipHostMallocPortable) != hipSuccess) {
        (void) hipGetLastError();
        *memory = nullptr;
        push_error(0x33B, "Failed to allocate %lld bytes of page-locked memory.", (long long) num_bytes);
        return PV_STATUS_OUT_OF_MEMORY;
    }
    return PV_STATUS_SUCCESS;
}

PV_API void pv_koala_batch_host_free(void *memory) {
    if (memory) (void) hipHostFree(memory);
}

PV_API pv_status_t pv_koala_batch_synchronize(pv_koala_batch_t *object) {
    t_stack.clear();
    if (!object) return check_object(object);
    std::string err;
    if (!object->engine->synchronize(&err)) {
        push_error(0x339, "%s", err.c_str());
        return PV_STATUS_RUNTIME_ERROR;
    }
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_profile_enable(pv_koala_batch_t *object, int32_t enable) {
    t_stack.clear();
    if (!object) return check_object(object);
    object->engine->profile_enable(enable != 0);
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_profile_read(pv_koala_batch_t *object, double *milliseconds, int64_t *launches) {
    t_stack.clear();
    if (!object || !milliseconds || !launches) {
        push_error(0x64, "Argument is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    std::string err;
    if (!object->engine->profile_read(milliseconds, launches, &err)) {
        push_error(0x339, "%s", err.c_str());
        return PV_STATUS_RUNTIME_ERROR;
    }
    return PV_STATUS_SUCCESS;
}

PV_API int64_t pv_koala_batch_debug_read(pv_koala_batch_t *object, int32_t what, float *out, int64_t capacity) {
    t_stack.clear();
    if (!object || !out) return -(int64_t) PV_STATUS_INVALID_ARGUMENT;
    std::string err;
    int64_t n = -1;
    try {
        n = object->engine->debug_read(what, out, capacity, &err);
    } catch (...) {
        err = "Failed to allocate memory.";
    }
    if (n < 0) {
        push_error(0x33A, "%s", n == -2 ? "capacity too small" : err.c_str());
        return -(int64_t) PV_STATUS_INVALID_ARGUMENT;
    }
    return n;
}

#ifdef KNS_TIMING
PV_API void pv_koala_debug_timing(unsigned long long *out) { kns::read_timing(out); }
#endif

}  // extern "C"
