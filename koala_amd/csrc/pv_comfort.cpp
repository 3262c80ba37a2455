// pv_comfort.cpp -- the C ABI of comfort noise (include/pv_koala_batch.h, COMFORT NOISE; DESIGN.md section 2, twelfth extension):
// pv_koala_batch_set_comfort_noise / _get_comfort_noise, pv_koala_batch_get_comfort_state / _set_comfort_state,
// pv_koala_set_comfort_noise / _get_comfort_noise.  The setting and the amplitude curves are the handle's (pv_api_internal.h,
// HandleSettings::comfort) and travel with every call; the frame counters are the engine's.
#include <cmath>

#include "pv_api_internal.h"

using kns_api::push_error;

namespace {

constexpr int32_t kSize = (int32_t) sizeof(pv_koala_comfort_t);
constexpr int K = PV_KOALA_NUM_BINS, R = kns::kComfortRow;

// pv_koala_batch_set_comfort_noise / pv_koala_set_comfort_noise (kns_api::set_table: every entry and every bin is checked before anything is
// changed).  The amplitude rows and the neutral band profile are prepared beside the table and swapped in once it is accepted.
pv_status_t set_comfort(HandleSettings *h, int32_t B, int32_t count, const int32_t *streams, const pv_koala_comfort_t *settings, const float *amplitude) {
    return kns_api::guarded([&] {
        std::vector<float> amp(h->comfort_amp), profile;
        if (amp.empty()) amp.assign((size_t) B * R, 0.0f);
        if (h->profile.empty()) {  // the neutral band profile: the comfort kernels carry the profile's clamp, so the call carries a table
            profile.assign((size_t) B * kns::kProfileRow, 0.0f);
            for (int32_t b = 0; b < B; ++b)
                for (int k = 0; k < K; ++k) profile[(size_t) b * kns::kProfileRow + kns::profile_index(k, 1)] = 1.0f;
        }
        const pv_status_t status = kns_api::set_table(
            &h->comfort, &h->comfort_any, &h->comfort_rev, kns::ComfortSetting{0, 0u}, B, count, streams, settings, "pv_koala_comfort_t", "comfort", "entry 0",
            [&](int32_t i, int32_t b, const pv_koala_comfort_t &s, kns::ComfortSetting *to) {
                if (s.on != 0 && s.on != 1) {
                    push_error(0x66, "comfort %d: `on` %d is not 0 or 1.", i, s.on);
                    return false;
                }
                *to = kns::ComfortSetting{s.on, s.seed};
                for (int k = 0; amplitude && k < K; ++k) {
                    const float a = amplitude[(size_t) i * K + k];
                    if (!(a >= 0.0f) || !std::isfinite(a)) {  // (NaN fails the comparison)
                        push_error(0x66, "comfort %d, bin %d: amplitude %g is not finite and >= 0.", i, k, (double) a);
                        return false;
                    }
                    amp[(size_t) b * R + kns::comfort_index(k)] = a + 0.0f;  // (-0 -> +0)
                }
                return true;
            });
        if (status != PV_STATUS_SUCCESS) return status;
        if (!profile.empty()) h->profile.swap(profile);
        h->comfort_amp.swap(amp);
        return status;
    });
}

pv_status_t get_comfort(const HandleSettings &h, int32_t b, pv_koala_comfort_t *setting, float *amplitude) {
    if (setting && !kns_api::getter_size_ok(setting->struct_size, kSize, "pv_koala_comfort_t")) return PV_STATUS_INVALID_ARGUMENT;
    const bool set = !h.comfort.empty();
    if (setting) {
        setting->on = set ? h.comfort[(size_t) b].on : 0;
        setting->seed = set ? h.comfort[(size_t) b].seed : 0u;
    }
    for (int k = 0; amplitude && k < K; ++k) amplitude[k] = set ? h.comfort_amp[(size_t) b * R + kns::comfort_index(k)] : 0.0f;
    return PV_STATUS_SUCCESS;
}

pv_status_t comfort_state(pv_koala_batch_t *object, bool set, int32_t count, const int32_t *streams, uint32_t *n) {
    return kns_api::stage_state(object, set, count, streams, n, "n", [](int32_t) { return true; }, &kns::Engine::comfort_state, 0x33F);
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
    return set_comfort(&object->settings, object->engine->num_streams(), count, streams, settings, amplitude);
}

PV_API pv_status_t pv_koala_batch_get_comfort_noise(const pv_koala_batch_t *object, int32_t stream, pv_koala_comfort_t *setting, float *amplitude) {
    kns_api::clear_errors();
    if (!object) return null_object();
    if (stream < 0 || stream >= object->engine->num_streams()) {
        push_error(0x66, "`stream` %d is outside [0, %d).", stream, object->engine->num_streams());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return get_comfort(object->settings, stream, setting, amplitude);
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
    return set_comfort(&object->settings, 1, 1, nullptr, setting, amplitude);
}

PV_API pv_status_t pv_koala_get_comfort_noise(const pv_koala_t *object, pv_koala_comfort_t *setting, float *amplitude) {
    kns_api::clear_errors();
    if (!object) return null_object();
    return get_comfort(object->settings, 0, setting, amplitude);
}
