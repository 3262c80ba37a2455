// pv_level.cpp -- the C ABI of the output leveller (include/pv_koala_batch.h, OUTPUT LEVELLER; DESIGN.md section 2, eleventh extension):
// pv_koala_batch_set_level / _get_level, pv_koala_batch_get_level_state / _set_level_state, pv_koala_set_level / _get_level.  The setting is
// the handle's (pv_api_internal.h, HandleSettings::level) and travels with every call; the state is the engine's.
#include <cmath>

#include "pv_api_internal.h"

using kns_api::push_error;

namespace {

constexpr int32_t kSize = (int32_t) sizeof(pv_koala_level_t);

// one setting, field by field: the first failure's message
bool check_setting(int32_t i, const pv_koala_level_t &s) {
    if (s.on != 0 && s.on != 1) {
        push_error(0x66, "setting %d: `on` %d is not 0 or 1.", i, s.on);
        return false;
    }
    const struct {
        const char *name;
        float v;
        bool ok;
        const char *want;
    } fields[] = {
        {"target", s.target, s.target > 0.0f, "an energy > 0"},
        {"max_boost", s.max_boost, s.max_boost >= 1.0f, "a gain >= 1"},
        {"max_cut", s.max_cut, s.max_cut > 0.0f && s.max_cut <= 1.0f, "a gain in (0, 1]"},
        {"theta", s.theta, s.theta >= 0.0f && s.theta <= 1.0f, "a mean mask in [0, 1]"},
        {"e_floor", s.e_floor, s.e_floor >= 0.0f, "an energy >= 0"},
        {"a_up", s.a_up, s.a_up > 0.0f && s.a_up <= 1.0f, "a coefficient in (0, 1]"},
        {"a_down", s.a_down, s.a_down > 0.0f && s.a_down <= 1.0f, "a coefficient in (0, 1]"},
        {"slew", s.slew, s.slew > 0.0f && s.slew <= 1.0f, "a coefficient in (0, 1]"},
    };
    for (const auto &f : fields)
        if (!f.ok || !std::isfinite(f.v)) {  // (NaN fails every comparison)
            push_error(0x66, "setting %d: `%s` %g is not %s.", i, f.name, (double) f.v, f.want);
            return false;
        }
    return true;
}

// what a handle holds for a stream until its first accepted change: off, and fields that would be accepted as they are
kns::LevelSetting neutral() { return kns::LevelSetting{0, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f, 1.0f, 1.0f, 1.0f}; }

// pv_koala_batch_set_level / pv_koala_set_level (kns_api::set_table: every entry is checked before anything is changed)
pv_status_t set_level(HandleSettings *h, int32_t B, int32_t count, const int32_t *streams, const pv_koala_level_t *settings) {
    return kns_api::set_table(&h->level, &h->level_any, &h->level_rev, neutral(), B, count, streams, settings, "pv_koala_level_t", "setting", "setting 0",
                              [](int32_t i, int32_t, const pv_koala_level_t &s, kns::LevelSetting *to) {
                                  if (!check_setting(i, s)) return false;
                                  *to = kns::LevelSetting{s.on, s.target, s.max_boost, s.max_cut, s.theta, s.e_floor + 0.0f, s.a_up, s.a_down, s.slew};
                                  return true;
                              });
}

pv_status_t get_level(const HandleSettings &h, int32_t b, pv_koala_level_t *setting) {
    if (!setting) {
        push_error(0x64, "Argument `setting` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!kns_api::getter_size_ok(setting->struct_size, kSize, "pv_koala_level_t")) return PV_STATUS_INVALID_ARGUMENT;
    const kns::LevelSetting s = h.level.empty() ? neutral() : h.level[(size_t) b];
    setting->on = s.on;
    setting->target = s.target, setting->max_boost = s.max_boost, setting->max_cut = s.max_cut, setting->theta = s.theta;
    setting->e_floor = s.e_floor, setting->a_up = s.a_up, setting->a_down = s.a_down, setting->slew = s.slew;
    return PV_STATUS_SUCCESS;
}

pv_status_t level_state(pv_koala_batch_t *object, bool set, int32_t count, const int32_t *streams, float *state) {
    const auto value_ok = [&](int32_t i) {
        const float lvl = state[2 * i], gain = state[2 * i + 1];
        if (!(lvl >= 0.0f) || !std::isfinite(lvl)) {
            push_error(0x66, "state %d: `lvl` %g is not an energy >= 0.", i, (double) lvl);
            return false;
        }
        if (!(gain > 0.0f) || !std::isfinite(gain)) {
            push_error(0x66, "state %d: `gain` %g is not a gain > 0.", i, (double) gain);
            return false;
        }
        return true;
    };
    return kns_api::stage_state(object, set, count, streams, state, "state", value_ok, &kns::Engine::level_state, 0x33E);
}

}  // namespace

PV_API pv_status_t pv_koala_batch_set_level(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const pv_koala_level_t *settings) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return set_level(&object->settings, object->engine->num_streams(), count, streams, settings);
}

PV_API pv_status_t pv_koala_batch_get_level(const pv_koala_batch_t *object, int32_t stream, pv_koala_level_t *setting) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (stream < 0 || stream >= object->engine->num_streams()) {
        push_error(0x66, "`stream` %d is outside [0, %d).", stream, object->engine->num_streams());
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return get_level(object->settings, stream, setting);
}

PV_API pv_status_t pv_koala_batch_get_level_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, float *state) {
    return level_state(object, false, count, streams, state);
}

PV_API pv_status_t pv_koala_batch_set_level_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const float *state) {
    return level_state(object, true, count, streams, const_cast<float *>(state));  // (read only when `set`)
}

PV_API pv_status_t pv_koala_set_level(pv_koala_t *object, const pv_koala_level_t *setting) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return set_level(&object->settings, 1, 1, nullptr, setting);
}

PV_API pv_status_t pv_koala_get_level(const pv_koala_t *object, pv_koala_level_t *setting) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    return get_level(object->settings, 0, setting);
}
