// pv_api_format.cpp -- the C ABI of sample formats (include/pv_koala_batch.h: pv_koala_batch_init_config, _sample_format; DESIGN.md section 2,
// fifth extension).  One struct-taking constructor over the three existing ones: with PV_KOALA_SAMPLE_S16 the handle is what they return; any
// other format is set on the engine behind the finished handle, whose processing entry points (pv_api.cpp, pv_api_packets.cpp) then take
// and deliver elements of that format through the pointers they have always had.
#include "pv_api_internal.h"

using kns_api::push_error;

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
    const pv_status_t st =
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
