// pv_limiter.cpp -- the C ABI of the peak limiter (include/pv_koala_batch.h, PEAK LIMITER; DESIGN.md section 2, thirteenth extension):
// pv_koala_batch_set_limiter / _get_limiter, pv_koala_batch_get_limiter_state / _set_limiter_state, pv_koala_set_limiter / _get_limiter.
// The setting is the handle's (pv_api_internal.h, HandleSettings::limiter) and travels with every call; the state is the engine's.
#include <cmath>

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

// pv_koala_batch_set_limiter / pv_koala_set_limiter (kns_api::set_table: every entry is checked before anything is changed)
pv_status_t set_limiter(HandleSettings *h, int32_t B, int32_t count, const int32_t *streams, const pv_koala_limiter_t *settings) {
    return kns_api::set_table(&h->limiter, &h->limiter_any, &h->limiter_rev, neutral(), B, count, streams, settings, "pv_koala_limiter_t", "setting",
                              "setting 0", [](int32_t i, int32_t, const pv_koala_limiter_t &s, kns::LimiterSetting *to) {
                                  if (!check_setting(i, s)) return false;
                                  *to = kns::LimiterSetting{s.on, s.ceiling, s.release};
                                  return true;
                              });
}

pv_status_t get_limiter(const HandleSettings &h, int32_t b, pv_koala_limiter_t *setting) {
    if (!setting) {
        push_error(0x64, "Argument `setting` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!kns_api::getter_size_ok(setting->struct_size, kSize, "pv_koala_limiter_t")) return PV_STATUS_INVALID_ARGUMENT;
    const kns::LimiterSetting s = h.limiter.empty() ? neutral() : h.limiter[(size_t) b];
    setting->on = s.on, setting->ceiling = s.ceiling, setting->release = s.release;
    return PV_STATUS_SUCCESS;
}

pv_status_t limiter_state(pv_koala_batch_t *object, bool set, int32_t count, const int32_t *streams, float *state) {
    const auto value_ok = [&](int32_t i) {
        if (state[i] > 0.0f && state[i] <= 1.0f) return true;  // (NaN fails every comparison)
        push_error(0x66, "state %d: `g` %g is not a gain in (0, 1].", i, (double) state[i]);
        return false;
    };
    return kns_api::stage_state(object, set, count, streams, state, "state", value_ok, &kns::Engine::limiter_state, 0x340);
}

}  // namespace

PV_API pv_status_t pv_koala_batch_set_limiter(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const pv_koala_limiter_t *settings) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return set_limiter(&object->settings, object->engine->num_streams(), count, streams, settings);
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
    return get_limiter(object->settings, stream, setting);
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
    return set_limiter(&object->settings, 1, 1, nullptr, setting);
}

PV_API pv_status_t pv_koala_get_limiter(const pv_koala_t *object, pv_koala_limiter_t *setting) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return get_limiter(object->settings, 0, setting);
}
