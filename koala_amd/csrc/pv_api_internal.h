// pv_api_internal.h -- what the translation units of the C ABI share: the handles behind the opaque pointers, the calling thread's error
// stack and the exception barrier.  pv_api.cpp owns all of it; pv_api_extensions.cpp (packet handles, sample formats, channels and their link) pv_level.cpp (the output leveller), pv_limiter.cpp (the peak limiter) and pv_comfort.cpp (comfort noise) use it.
// Nothing here leaves the library.
#pragma once

#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pv_koala.h"
#include "../../include/pv_koala_batch.h"
#include "kns_engine.h"

// The attenuation limit of a handle (include/pv_koala_batch.h, pv_koala_batch_set_min_gain): configuration that the handle owns and every
// call carries to the engine (kns::Call::min_gain) -- the engine keeps nothing of it between calls but its device table.
struct MinGain {
    std::vector<float> gain;  // [num_streams], every value in [0, 1]
    unsigned rev = 0;         // counts the accepted changes: the engine uploads the table when it has not seen this one
    bool any = false;         // some gain is non-zero (none: the calls are the plain calls, no table at all)
    // Linked channels (pv_koala_batch_set_channel_link; batch handles only): travels with the limit because a linked call carries the gains
    // whether or not any is non-zero -- the linked kernels read the table (kns::Call::channel_link)
    int link = 0;
    // High-band carry (pv_koala_batch_set_high_band; frame handles at 32 and 48 kHz only): the mode, and the number of times it was turned
    // on -- the engine clears the feature's state when it sees a new one (kns::Call::high_band, high_band_epoch).  Travels with the limit
    // because every call that advances the streams passes through it.
    int high_band = 0;
    unsigned high_band_epoch = 0;
    // Band profile (pv_koala_batch_set_band_profile): every stream's floors and ceilings [num_streams][kns::kProfileRow] in the order the
    // engine's table has them (kns::profile_index), empty until the first accepted change; its revision counter, like `rev`; and whether
    // any stream's profile is not the neutral one (none: the calls are the plain calls, no table at all).  Travels with the limit for the
    // reason above (kns::Call::band_profile)
    std::vector<float> profile;
    unsigned profile_rev = 0;
    bool profile_any = false;
    // Output leveller (pv_koala_batch_set_level; pv_level.cpp): every stream's setting [num_streams], empty until the first accepted
    // change; its revision counter, like `rev`; and whether any stream's leveller is on (none: the calls are the plain calls, no table at
    // all).  Travels with the limit for the reason above (kns::Call::level).  The leveller's STATE is the engine's.
    std::vector<kns::LevelSetting> level;
    unsigned level_rev = 0;
    bool level_any = false;
    // Peak limiter (pv_koala_batch_set_limiter; pv_limiter.cpp): the same three for it (kns::Call::limiter).  Its STATE, g, is the engine's.
    std::vector<kns::LimiterSetting> limiter;
    unsigned limiter_rev = 0;
    bool limiter_any = false;
    // Comfort noise (pv_koala_batch_set_comfort_noise; pv_comfort.cpp): every stream's setting [num_streams] and amplitude curve
    // [num_streams][kns::kComfortRow] in the order the engine's table has them (kns::comfort_index), empty until the first accepted change;
    // one revision counter for both; and whether any stream's comfort noise is on (none: the calls are the plain calls, no table at all).
    // A call with comfort noise carries `gain` and `profile` too (pv_comfort.cpp makes `profile` the neutral table when it is still empty):
    // the comfort kernels read both.  The frame COUNTERS are the engine's.
    std::vector<kns::ComfortSetting> comfort;
    std::vector<float> comfort_amp;
    unsigned comfort_rev = 0;
    bool comfort_any = false;
};
struct pv_koala {
    kns::Engine *engine;
    MinGain limit;
};
struct pv_koala_batch {
    kns::Engine *engine;
    MinGain limit;
    int32_t sample_rate = kns::kRate16k;  // fixed at creation (pv_koala_batch_init_rate); the engine was made with the same value
    int32_t packet_samples = 0;           // a packet handle's max_samples_per_call (pv_koala_batch_init_packets); 0: a frame handle
    // (both are the CALLER's values: on a handle at 44 100 or 22 050 Hz the engine's are those of the 16 kHz packet engine inside.  The
    // sample format and the channels are the engine's alone: engine->sample_format(), engine->channels())
};

namespace kns_api {

void clear_errors();                                   // every entry point first: the calling thread's error stack is emptied
void push_error(unsigned code, const char *fmt, ...);  // one message onto it (at most 8 are kept)
// A call under a band profile that is not neutral: what it is not combined with yet (PV_STATUS_INVALID_ARGUMENT and a message), else SUCCESS
pv_status_t check_band_profile(const MinGain &limit);
// A call while some stream's leveller is on: what it is not combined with yet -- the channel link, the high-band carry, the asynchronous
// entry points, a handle at 44 100 or 22 050 Hz (PV_STATUS_INVALID_ARGUMENT and a message), else SUCCESS
pv_status_t check_level(const MinGain &limit, const kns::Engine *engine, bool async);
// A call while some stream's limiter is on: the same four refusals, else SUCCESS; carry_limiter: what such a call takes to the engine
pv_status_t check_limiter(const MinGain &limit, const kns::Engine *engine, bool async);
template <class C>
void carry_limiter(const MinGain &limit, C *call) {
    if (limit.limiter_any) call->limiter = limit.limiter.data(), call->limiter_rev = limit.limiter_rev;
}
// A call while some stream's comfort noise is on: the same four refusals, else SUCCESS; carry_comfort: what such a call takes to the engine
pv_status_t check_comfort(const MinGain &limit, const kns::Engine *engine, bool async);
template <class C>
void carry_comfort(const MinGain &limit, C *call) {
    if (!limit.comfort_any) return;
    call->comfort = limit.comfort.data(), call->comfort_amp = limit.comfort_amp.data(), call->comfort_rev = limit.comfort_rev;
    call->min_gain = limit.gain.data(), call->min_gain_rev = limit.rev;
    call->band_profile = limit.profile.data(), call->band_profile_rev = limit.profile_rev;
}
// what an engine call that did not succeed leaves on the stack: a refused argument, or a failure under the entry point's own code
pv_status_t engine_failure(kns::Status status, unsigned runtime_code, const std::string &err);

// No C++ exception may cross the C ABI (the callers are ctypes / dlsym hosts: an escaping exception is std::terminate).  Every
// entry point that reaches engine code runs it through this: bad_alloc -> OUT_OF_MEMORY, anything else -> RUNTIME_ERROR.
template <class F>
pv_status_t guarded(F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        push_error(0x65, "Failed to allocate memory.");
        return PV_STATUS_OUT_OF_MEMORY;
    } catch (const std::length_error &) {
        push_error(0x65, "Failed to allocate memory.");
        return PV_STATUS_OUT_OF_MEMORY;
    } catch (const std::exception &e) {
        push_error(0x339, "Unexpected failure: %s", e.what());
        return PV_STATUS_RUNTIME_ERROR;
    } catch (...) {
        push_error(0x339, "Unexpected failure.");
        return PV_STATUS_RUNTIME_ERROR;
    }
}

}  // namespace kns_api
