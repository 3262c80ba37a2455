// pv_api_format.cpp -- the C ABI of sample formats (include/pv_koala_batch.h: pv_koala_batch_init_config, _sample_format; DESIGN.md section 2,
// fifth extension).  One struct-taking constructor over the three existing ones: with PV_KOALA_SAMPLE_S16 the handle is what they return; any
// other format is set on the engine behind the finished handle, whose processing entry points (pv_api.cpp, pv_api_packets.cpp) then take
// and deliver elements of that format through the pointers they have always had.
#include "pv_api_internal.h"

using kns_api::push_error;

// A handle at 44 100 or 22 050 Hz (sixth extension): always a packet handle -- there is no whole frame at such a rate.
// It is a 16 kHz packet handle that takes the most inner samples a call can yield, ceil(U max_samples_per_call / 441), with the fractional
// stages enabled around its packet call; sample_rate and packet_samples of the handle are the caller's.
static pv_status_t init_fractional(const char *access_key, const char *model_path, const char *device, const pv_koala_batch_config_t *config,
                                   pv_koala_precision_t precision, pv_koala_batch_t **object) {
    const int32_t rate = config->sample_rate, max_samples = config->max_samples_per_call;
    if (max_samples <= 0) {
        push_error(0x66, "`sample_rate` %d needs `max_samples_per_call` > 0: a handle at this rate must be a packet handle (16 ms is not a "
                         "whole number of samples there).", rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (max_samples > kns::kFrMaxSamples) {
        push_error(0x66, "`max_samples_per_call` %d is above %d, the most a handle whose `sample_rate` is %d takes.", max_samples,
                   kns::kFrMaxSamples, rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const int32_t inner_max = (int32_t) kns::fr_inner(max_samples, kns::fr_up(rate));
    const pv_status_t st = pv_koala_batch_init_packets(access_key, model_path, device, config->num_streams, inner_max, precision, kns::kRate16k, object);
    if (st != PV_STATUS_SUCCESS) return st;
    return kns_api::guarded([&] {
        std::string err;
        if (!(*object)->engine->enable_fractional(rate, max_samples, &err)) {
            pv_koala_batch_delete(*object);
            *object = nullptr;
            push_error(0x65, "%s", err.c_str());
            return PV_STATUS_OUT_OF_MEMORY;
        }
        (*object)->sample_rate = rate;
        (*object)->packet_samples = max_samples;
        return PV_STATUS_SUCCESS;
    });
}

PV_API pv_status_t pv_koala_batch_init_config(const char *access_key, const char *model_path, const char *device,
                                              const pv_koala_batch_config_t *config, pv_koala_batch_t **object) {
    kns_api::clear_errors();
    if (!config) {
        push_error(0x64, "Argument `config` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (config->struct_size != (int32_t) sizeof(pv_koala_batch_config_t)) {
        push_error(0x66, "`struct_size` %d is not sizeof(pv_koala_batch_config_t) = %d.", config->struct_size, (int) sizeof(pv_koala_batch_config_t));
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!kns::fmt_ok(config->sample_format)) {
        push_error(0x66, "`sample_format` %d is not one of PV_KOALA_SAMPLE_S16, _F32, _ULAW, _ALAW (0 ... 3).", config->sample_format);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (config->precision != PV_KOALA_PRECISION_FP32 && config->precision != PV_KOALA_PRECISION_BF16) {
        push_error(0x66, "`precision` must be PV_KOALA_PRECISION_FP32 or PV_KOALA_PRECISION_BF16.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const pv_koala_precision_t precision = config->precision == PV_KOALA_PRECISION_BF16 ? PV_KOALA_PRECISION_BF16 : PV_KOALA_PRECISION_FP32;
    if (config->sample_rate == 11025) {
        push_error(0x66, "`sample_rate` 11025 is not available yet: of the 44 100 Hz family, 44100 and 22050 are.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const bool fractional = kns::fr_rate_ok(config->sample_rate);
    if (fractional) {
        const pv_status_t made = init_fractional(access_key, model_path, device, config, precision, object);
        if (made != PV_STATUS_SUCCESS) return made;
    }
    const pv_status_t st =
        fractional ? PV_STATUS_SUCCESS :
        config->max_samples_per_call > 0
            ? pv_koala_batch_init_packets(access_key, model_path, device, config->num_streams, config->max_samples_per_call, precision,
                                          config->sample_rate, object)
            : pv_koala_batch_init_rate(access_key, model_path, device, config->num_streams, config->max_frames_per_call, precision,
                                       config->sample_rate, object);
    if (st != PV_STATUS_SUCCESS || config->sample_format == PV_KOALA_SAMPLE_S16) return st;
    return kns_api::guarded([&] {
        std::string err;
        if (!(*object)->engine->set_format(config->sample_format, &err)) {
            pv_koala_batch_delete(*object);
            *object = nullptr;
            push_error(0x65, "%s", err.c_str());
            return PV_STATUS_OUT_OF_MEMORY;
        }
        (*object)->sample_format = config->sample_format;
        return PV_STATUS_SUCCESS;
    });
}

PV_API pv_status_t pv_koala_batch_sample_format(const pv_koala_batch_t *object, int32_t *sample_format) {
    kns_api::clear_errors();
    if (!object || !sample_format) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "sample_format" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *sample_format = object->sample_format;
    return PV_STATUS_SUCCESS;
}
