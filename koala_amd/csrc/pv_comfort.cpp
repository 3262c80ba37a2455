// pv_comfort.cpp -- the C ABI of comfort noise (include/pv_koala_batch.h, COMFORT NOISE; DESIGN.md section 2, twelfth extension):
// pv_koala_batch_set_comfort_noise / _get_comfort_noise, pv_koala_batch_get_comfort_state / _set_comfort_state,
// pv_koala_set_comfort_noise / _get_comfort_noise.  The setting and the amplitude curves are the handle's (pv_api_internal.h,
// MinGain::comfort) and travel with every call; the frame counters are the engine's.
#include <cmath>
#include <string.h>

#include "pv_api_internal.h"

using kns_api::push_error;

namespace {

constexpr int32_t kSize = (int32_t) sizeof(pv_koala_comfort_t);
constexpr int K = PV_KOALA_NUM_BINS, R = kns::kComfortRow;

// pv_koala_batch_set_comfort_noise / pv_koala_set_comfort_noise: every entry and every bin is checked before anything is changed
pv_status_t set_comfort(MinGain *limit, int32_t B, int32_t count, const int32_t *streams, const pv_koala_comfort_t *settings, const float *amplitude) {
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
        push_error(0x66, "`struct_size` %d is not sizeof(pv_koala_comfort_t) = %d (or more, in whole words, from a later header).", stride, kSize);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return kns_api::guarded([&] {
        std::vector<kns::ComfortSetting> next(limit->comfort);
        std::vector<float> amp(limit->comfort_amp);
        if (next.empty()) next.assign((size_t) B, kns::ComfortSetting{0, 0u});
        if (amp.empty()) amp.assign((size_t) B * R, 0.0f);
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
            pv_koala_comfort_t s;
            memcpy(&s, (const char *) settings + (size_t) i * stride, sizeof(s));
            if (s.struct_size != stride) {
                push_error(0x66, "comfort %d: `struct_size` %d differs from that of entry 0, %d.", i, s.struct_size, stride);
                return PV_STATUS_INVALID_ARGUMENT;
            }
            if (s.on != 0 && s.on != 1) {
                push_error(0x66, "comfort %d: `on` %d is not 0 or 1.", i, s.on);
                return PV_STATUS_INVALID_ARGUMENT;
            }
            next[b] = kns::ComfortSetting{s.on, s.seed};
            for (int k = 0; amplitude && k < K; ++k) {
                const float a = amplitude[(size_t) i * K + k];
                if (!(a >= 0.0f) || !std::isfinite(a)) {  // (NaN fails the comparison)
                    push_error(0x66, "comfort %d, bin %d: amplitude %g is not finite and >= 0.", i, k, (double) a);
                    return PV_STATUS_INVALID_ARGUMENT;
                }
                amp[(size_t) b * R + kns::comfort_index(k)] = a + 0.0f;  // (-0 -> +0)
            }
        }
        bool any = false;
        for (const kns::ComfortSetting &s : next) any = any || s.on != 0;
        std::vector<float> profile;
        if (limit->profile.empty()) {  // the neutral band profile: the comfort kernels carry the profile's clamp, so the call carries a table
            profile.assign((size_t) B * kns::kProfileRow, 0.0f);
            for (int32_t b = 0; b < B; ++b)
                for (int k = 0; k < K; ++k) profile[(size_t) b * kns::kProfileRow + kns::profile_index(k, 1)] = 1.0f;
        }
        if (!profile.empty()) limit->profile.swap(profile);  // (nothing below throws)
        limit->comfort.swap(next);
        limit->comfort_amp.swap(amp);
        limit->comfort_any = any;
        ++limit->comfort_rev;
        return PV_STATUS_SUCCESS;
    });
}

pv_status_t get_comfort(const MinGain &limit, int32_t b, pv_koala_comfort_t *setting, float *amplitude) {
    if (setting && setting->struct_size < kSize) {
        push_error(0x66, "`struct_size` %d is not sizeof(pv_koala_comfort_t) = %d (or more, from a later header).", setting->struct_size, kSize);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const bool set = !limit.comfort.empty();
    if (setting) {
        setting->on = set ? limit.comfort[(size_t) b].on : 0;
        setting->seed = set ? limit.comfort[(size_t) b].seed : 0u;
    }
    for (int k = 0; amplitude && k < K; ++k) amplitude[k] = set ? limit.comfort_amp[(size_t) b * R + kns::comfort_index(k)] : 0.0f;
    return PV_STATUS_SUCCESS;
}

pv_status_t comfort_state(pv_koala_batch_t *object, bool set, int32_t count, const int32_t *streams, uint32_t *n) {
    kns_api::clear_errors();
    if (!object || !n) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "n" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const int32_t B = object->engine->num_streams();
    if (count < 1 || count > B) {
        push_error(0x66, "`count` %d is outside [1, %d].", count, B);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return kns_api::guarded([&] {
        std::string err;
        const kns::Status status = object->engine->comfort_state(set, count, streams, n, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : kns_api::engine_failure(status, 0x33F, err);
    });
}

pv_status_t null_object() {
    push_error(0x64, "Argument `object` is NULL.");
    return PV_STATUS_INVALID_ARGUMENT;
}

}  // namespace

PV_API pv_status_t pv_koala_batch_set_comfort_noise(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const pv_koala_comfort_t *settings,
                                                    const float *amplitude) {
    kns_api::clear_errors();
    if (!object) return null_object();
    return set_comfort(&object->limit, object->engine->num_streams(), count, streams, settings, amplitude);
}

PV_API pv_status_t pv_koala_batch_get_comfort_noise(const pv_koala_batch_t *object, int32_t stream, pv_koala_comfort_t *setting, float *amplitude) {
    kns_api::clear_errors();
    if (!object) return null_object();
    if (stream < 0 || stream >= object->engine->num_streams()) {
        push_error(0x66, "`stream` %d is outside [0, %d).", stream, object->engine->num_streams());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return get_comfort(object->limit, stream, setting, amplitude);
}

PV_API pv_status_t pv_koala_batch_get_comfort_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, uint32_t *n) {
    return comfort_state(object, false, count, streams, n);
}

PV_API pv_status_t pv_koala_batch_set_comfort_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const uint32_t *n) {
    return comfort_state(object, true, count, streams, const_cast<uint32_t *>(n));  // (read only when `set`)
}

PV_API pv_status_t pv_koala_set_comfort_noise(pv_koala_t *object, const pv_koala_comfort_t *setting, const float *amplitude) {
    kns_api::clear_errors();
    if (!object) return null_object();
    return set_comfort(&object->limit, 1, 1, nullptr, setting, amplitude);
}

PV_API pv_status_t pv_koala_get_comfort_noise(const pv_koala_t *object, pv_koala_comfort_t *setting, float *amplitude) {
    kns_api::clear_errors();
    if (!object) return null_object();
    return get_comfort(object->limit, 0, setting, amplitude);
}
