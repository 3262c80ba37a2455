// pv_limiter.cpp -- the C ABI of the peak limiter (include/pv_koala_batch.h, PEAK LIMITER; DESIGN.md section 2, thirteenth extension):
// pv_koala_batch_set_limiter / _get_limiter, pv_koala_batch_get_limiter_state / _set_limiter_state, pv_koala_set_limiter / _get_limiter.
// The setting is the handle's (pv_api_internal.h, MinGain::limiter) and travels with every call; the state is the engine's.
#include <cmath>
#include <string.h>

#include "pv_api_internal.h"

using kns_api::push_error;

namespace {

constexpr int32_t kSize = (int32_t) sizeof(pv_koala_limiter_t);

// one setting, field by field: the first failure's message
bool check_setting(int32_t i, const pv_koala_limiter_t &s) {
    if (s.on != 0 && s.on != 1) {
        push_error(0x66, "setting %d: `on` %d is not 0 or 1.", i, s.on);
        return false;
    }
    if (!(s.ceiling >= 1.0f && s.ceiling <= 32767.0f)) {  // (NaN fails every comparison)
        push_error(0x66, "setting %d: `ceiling` %g is not a sample value in [1, 32767].", i, (double) s.ceiling);
        return false;
    }
    if (!(s.release > 0.0f && s.release <= 1.0f)) {
        push_error(0x66, "setting %d: `release` %g is not a gain per sample in (0, 1].", i, (double) s.release);
        return false;
    }
    return true;
}

// what a handle holds for a stream until its first accepted change: off, and fields that would be accepted as they are
kns::LimiterSetting neutral() { return kns::LimiterSetting{0, 32767.0f, 1.0f}; }

// pv_koala_batch_set_limiter / pv_koala_set_limiter: every entry is checked before anything is changed
pv_status_t set_limiter(MinGain *limit, int32_t B, int32_t count, const int32_t *streams, const pv_koala_limiter_t *settings) {
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
        push_error(0x66, "`struct_size` %d is not sizeof(pv_koala_limiter_t) = %d (or more, in whole words, from a later header).", stride, kSize);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return kns_api::guarded([&] {
        std::vector<kns::LimiterSetting> next(limit->limiter);
        if (next.empty()) next.assign((size_t) B, neutral());
        std::vector<uint8_t> listed((size_t) B, 0);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t b = streams ? streams[i] : i;
            if (b < 0 || b >= B) {
                push_error(0x66, "`streams[%d]` = %d is outside [0, %d).", i, b, B);
                return PV_STATUS_INVALID_ARGUMENT;
            }
            if (listed[b]) {
                push_error(0x66, "`streams[%d]`: slot %d is listed twice.", i, b);
                return PV_STATUS_INVALID_ARGUMENT;
            }
            listed[b] = 1;
            pv_koala_limiter_t s;
            memcpy(&s, (const char *) settings + (size_t) i * stride, sizeof(s));
            if (s.struct_size != stride) {
                push_error(0x66, "setting %d: `struct_size` %d differs from that of setting 0, %d.", i, s.struct_size, stride);
                return PV_STATUS_INVALID_ARGUMENT;
            }
            if (!check_setting(i, s)) return PV_STATUS_INVALID_ARGUMENT;
            next[b] = kns::LimiterSetting{s.on, s.ceiling, s.release};
        }
        bool any = false;
        for (const kns::LimiterSetting &s : next) any = any || s.on != 0;
        limit->limiter.swap(next);
        limit->limiter_any = any;
        ++limit->limiter_rev;
        return PV_STATUS_SUCCESS;
    });
}

pv_status_t get_limiter(const MinGain &limit, int32_t b, pv_koala_limiter_t *setting) {
    if (!setting) {
        push_error(0x64, "Argument `setting` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (setting->struct_size < kSize) {
        push_error(0x66, "`struct_size` %d is not sizeof(pv_koala_limiter_t) = %d (or more, from a later header).", setting->struct_size, kSize);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const kns::LimiterSetting s = limit.limiter.empty() ? neutral() : limit.limiter[(size_t) b];
    setting->on = s.on, setting->ceiling = s.ceiling, setting->release = s.release;
    return PV_STATUS_SUCCESS;
}

pv_status_t limiter_state(pv_koala_batch_t *object, bool set, int32_t count, const int32_t *streams, float *state) {
    kns_api::clear_errors();
    if (!object || !state) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "state" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const int32_t B = object->engine->num_streams();
    if (count < 1 || count > B) {
        push_error(0x66, "`count` %d is outside [1, %d].", count, B);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    for (int32_t i = 0; set && i < count; ++i)
        if (!(state[i] > 0.0f && state[i] <= 1.0f)) {  // (NaN fails every comparison)
            push_error(0x66, "state %d: `g` %g is not a gain in (0, 1].", i, (double) state[i]);
            return PV_STATUS_INVALID_ARGUMENT;
        }
    return kns_api::guarded([&] {
        std::string err;
        const kns::Status status = object->engine->limiter_state(set, count, streams, state, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : kns_api::engine_failure(status, 0x340, err);
    });
}

}  // namespace

PV_API pv_status_t pv_koala_batch_set_limiter(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const pv_koala_limiter_t *settings) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return set_limiter(&object->limit, object->engine->num_streams(), count, streams, settings);
}

PV_API pv_status_t pv_koala_batch_get_limiter(const pv_koala_batch_t *object, int32_t stream, pv_koala_limiter_t *setting) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (stream < 0 || stream >= object->engine->num_streams()) {
        push_error(0x66, "`stream` %d is outside [0, %d).", stream, object->engine->num_streams());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return get_limiter(object->limit, stream, setting);
}

PV_API pv_status_t pv_koala_batch_get_limiter_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, float *state) {
    return limiter_state(object, false, count, streams, state);
}

PV_API pv_status_t pv_koala_batch_set_limiter_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const float *state) {
    return limiter_state(object, true, count, streams, const_cast<float *>(state));  // (read only when `set`)
}

PV_API pv_status_t pv_koala_set_limiter(pv_koala_t *object, const pv_koala_limiter_t *setting) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return set_limiter(&object->limit, 1, 1, nullptr, setting);
}

PV_API pv_status_t pv_koala_get_limiter(const pv_koala_t *object, pv_koala_limiter_t *setting) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return get_limiter(object->limit, 0, setting);
}
