// pv_api_internal.h -- what the translation units of the C ABI share: the handles behind the opaque pointers, the calling thread's error
// stack, the exception barrier, and the one path of a per-stream setting from an entry point to the call that carries it (DESIGN.md section
// 2, "Per-stream settings").  pv_api.cpp owns all of it; pv_api_extensions.cpp (packet handles, sample formats, channels and their link),
// pv_level.cpp (the output leveller), pv_limiter.cpp (the peak limiter) and pv_comfort.cpp (comfort noise) use it.
// Nothing here leaves the library.
#pragma once

#include <string.h>

#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pv_koala.h"
#include "../../include/pv_koala_batch.h"
#include "kns_engine.h"

// The settings of a handle: configuration that the handle owns and every call carries to the engine (kns::StreamOptions, filled by
// kns_api::carry) -- the engine keeps nothing of it between calls but its device tables.  First the attenuation limit
// (include/pv_koala_batch.h, pv_koala_batch_set_min_gain):
struct HandleSettings {
    std::vector<float> gain;  // [num_streams], every value in [0, 1]
    unsigned rev = 0;         // counts the accepted changes: the engine uploads the table when it has not seen this one
    bool any = false;         // some gain is non-zero (none: the calls are the plain calls, no table at all)
    // Linked channels (pv_koala_batch_set_channel_link; batch handles only): travels with the gains because a linked call carries the gains
    // whether or not any is non-zero -- the linked kernels read the table (kns::StreamOptions::channel_link)
    int link = 0;
    // High-band carry (pv_koala_batch_set_high_band; frame handles at 32 and 48 kHz only): the mode, and the number of times it was turned
    // on -- the engine clears the feature's state when it sees a new one (kns::Call::high_band, high_band_epoch).  Travels with the gains
    // because every call that advances the streams passes through it.
    int high_band = 0;
    unsigned high_band_epoch = 0;
    // Band profile (pv_koala_batch_set_band_profile): every stream's floors and ceilings [num_streams][kns::kProfileRow] in the order the
    // engine's table has them (kns::profile_index), empty until the first accepted change; its revision counter, like `rev`; and whether
    // any stream's profile is not the neutral one (none: the calls are the plain calls, no table at all).  Travels with the gains for the
    // reason above (kns::StreamOptions::band_profile)
    std::vector<float> profile;
    unsigned profile_rev = 0;
    bool profile_any = false;
    // Output leveller (pv_koala_batch_set_level; pv_level.cpp): every stream's setting [num_streams], empty until the first accepted
    // change; its revision counter, like `rev`; and whether any stream's leveller is on (none: the calls are the plain calls, no table at
    // all).  Travels with the gains for the reason above (kns::StreamOptions::level).  The leveller's STATE is the engine's.
    std::vector<kns::LevelSetting> level;
    unsigned level_rev = 0;
    bool level_any = false;
    // Peak limiter (pv_koala_batch_set_limiter; pv_limiter.cpp): the same three for it (kns::StreamOptions::limiter).  Its STATE, g, is the engine's.
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
    HandleSettings settings;
};
struct pv_koala_batch {
    kns::Engine *engine;
    HandleSettings settings;
    int32_t sample_rate = kns::kRate16k;  // fixed at creation (pv_koala_batch_init_rate); the engine was made with the same value
    int32_t packet_samples = 0;           // a packet handle's max_samples_per_call (pv_koala_batch_init_packets); 0: a frame handle
    // (both are the CALLER's values: on a handle at 44 100 or 22 050 Hz the engine's are those of the 16 kHz packet engine inside.  The
    // sample format and the channels are the engine's alone: engine->sample_format(), engine->channels())
};

namespace kns_api {

void clear_errors();                                   // every entry point first: the calling thread's error stack is emptied
void push_error(unsigned code, const char *fmt, ...);  // one message onto it (at most 8 are kept)
// A call under the handle's settings: what a band profile that is not neutral, the output leveller, the peak limiter and comfort noise -- in
// that order -- are not combined with yet (the channel link, the high-band carry; the three stages: the asynchronous entry points, a handle at
// 44 100 or 22 050 Hz): PV_STATUS_INVALID_ARGUMENT and a message, else SUCCESS
pv_status_t check_settings(const HandleSettings &s, const kns::Engine *engine, bool async);
// ... and what such a call takes to the engine.  The linked, the profile and the comfort kernels read the gains (all zero where no limit is
// in force), the comfort kernels the profile too (pv_comfort.cpp has made it the neutral table where none was set)
inline void carry(const HandleSettings &s, kns::StreamOptions *o) {
    if (s.any || s.link || s.profile_any || s.comfort_any) o->min_gain = s.gain.data(), o->min_gain_rev = s.rev;
    if (s.profile_any || s.comfort_any) o->band_profile = s.profile.data(), o->band_profile_rev = s.profile_rev;
    o->channel_link = s.link;
    if (s.level_any) o->level = s.level.data(), o->level_rev = s.level_rev;
    if (s.limiter_any) o->limiter = s.limiter.data(), o->limiter_rev = s.limiter_rev;
    if (s.comfort_any) o->comfort = s.comfort.data(), o->comfort_amp = s.comfort_amp.data(), o->comfort_rev = s.comfort_rev;
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


// ---- what the setters and getters of the per-stream settings share

// entry i of a stream list (nullptr: slot i) of a handle with listed->size() streams: the slot, marked; -1 and a message: outside the handle,
// or listed before
inline int32_t listed_stream(std::vector<uint8_t> *listed, const int32_t *streams, int32_t i) {
    const int32_t b = streams ? streams[i] : i, B = (int32_t) listed->size();
    if (b < 0 || b >= B) {
        push_error(0x66, "`streams[%d]` = %d is outside [0, %d).", i, b, B);
        return -1;
    }
    if ((*listed)[b]) {
        push_error(0x66, "`streams[%d]`: slot %d is listed twice.", i, b);
        return -1;
    }
    (*listed)[b] = 1;
    return b;
}

// A setter of `count` public structs Pub (their own `struct_size` apart: a later header's are longer) for the listed streams of a table of
// B internal settings Set, `neutral` until the first accepted change.  Every entry is checked before anything is changed:
// entry(i, b, pub, &set) checks entry i field by field, pushes the first failure's message and converts.  `type`: Pub's name; `noun`: what a
// message calls entry i ("setting", "comfort"); `first`: ... and entry 0.  Then the table is swapped, *any = some stream's `on`, ++*rev.
template <class Pub, class Set, class Entry>
pv_status_t set_table(std::vector<Set> *table, bool *any, unsigned *rev, const Set &neutral, int32_t B, int32_t count, const int32_t *streams,
                      const Pub *settings, const char *type, const char *noun, const char *first, Entry &&entry) {
    constexpr int32_t kSize = (int32_t) sizeof(Pub);
    if (!settings) {
        push_error(0x64, "Argument `settings` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (count < 1 || count > B) {
        push_error(0x66, "`count` %d is outside [1, %d].", count, B);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const int32_t stride = settings[0].struct_size;
    if (stride < kSize || stride % 4 != 0) {
        push_error(0x66, "`struct_size` %d is not sizeof(%s) = %d (or more, in whole words, from a later header).", stride, type, kSize);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return guarded([&] {
        std::vector<Set> next(*table);
        if (next.empty()) next.assign((size_t) B, neutral);
        std::vector<uint8_t> listed((size_t) B, 0);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t b = listed_stream(&listed, streams, i);
            if (b < 0) return PV_STATUS_INVALID_ARGUMENT;
            Pub s;
            memcpy(&s, (const char *) settings + (size_t) i * stride, sizeof(s));
            if (s.struct_size != stride) {
                push_error(0x66, "%s %d: `struct_size` %d differs from that of %s, %d.", noun, i, s.struct_size, first, stride);
                return PV_STATUS_INVALID_ARGUMENT;
            }
            if (!entry(i, b, s, &next[b])) return PV_STATUS_INVALID_ARGUMENT;
        }
        *any = false;
        for (const Set &s : next) *any = *any || s.on != 0;
        table->swap(next);
        ++*rev;
        return PV_STATUS_SUCCESS;
    });
}

// a getter's struct: its `struct_size` covers what this header knows
inline bool getter_size_ok(int32_t struct_size, int32_t size, const char *type) {
    if (struct_size >= size) return true;
    push_error(0x66, "`struct_size` %d is not sizeof(%s) = %d (or more, from a later header).", struct_size, type, size);
    return false;
}

// pv_koala_batch_get_*_state / _set_*_state: `arg` names the values' argument, value_ok(i) checks entry i of a set and pushes its message,
// `state` is the engine's accessor and `code` the entry point's own failure code
template <class T, class Check>
pv_status_t stage_state(pv_koala_batch *object, bool set, int32_t count, const int32_t *streams, T *values, const char *arg, Check &&value_ok,
                        kns::Status (kns::Engine::*state)(bool, int, const int32_t *, T *, std::string *), unsigned code) {
    clear_errors();
    if (!object || !values) {
        push_error(0x64, "Argument `%s` is NULL.", object ? arg : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const int32_t B = object->engine->num_streams();
    if (count < 1 || count > B) {
        push_error(0x66, "`count` %d is outside [1, %d].", count, B);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    for (int32_t i = 0; set && i < count; ++i)
        if (!value_ok(i)) return PV_STATUS_INVALID_ARGUMENT;
    return guarded([&] {
        std::string err;
        const kns::Status status = (object->engine->*state)(set, count, streams, values, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : engine_failure(status, code, err);
    });
}

}  // namespace kns_api
