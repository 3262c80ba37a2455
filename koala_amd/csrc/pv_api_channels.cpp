// pv_api_channels.cpp -- the C ABI of multi-channel batch handles (include/pv_koala_batch.h: pv_koala_batch_init_channels, _channels;
// DESIGN.md section 2, seventh extension).  One constructor over pv_koala_batch_init_config (pv_api_format.cpp): with channels == 1 the
// handle is what that returns; any other count is set on the engine behind the finished handle, whose processing entry points (pv_api.cpp,
// pv_api_packets.cpp) then take and deliver interleaved group rows through the pointers they have always had.  A translation unit of its
// own: the host-only builds of the other three (tests/abi_*) link without the engine member this one calls.
#include "pv_api_internal.h"

using kns_api::push_error;

// The layout of `pcm` and `enhanced`, set like the sample format and outside it.  The config struct does not grow: the count is an argument.
PV_API pv_status_t pv_koala_batch_init_channels(const char *access_key, const char *model_path, const char *device,
                                                const pv_koala_batch_config_t *config, int32_t channels, pv_koala_batch_t **object) {
    kns_api::clear_errors();
    if (channels < 1 || channels > kns::kChannelsMax) {
        push_error(0x66, "`channels` %d is outside [1, %d].", channels, kns::kChannelsMax);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (channels > 1 && config && config->struct_size == (int32_t) sizeof(pv_koala_batch_config_t) && config->num_streams > 0 &&
        config->num_streams % channels != 0) {
        push_error(0x66, "`num_streams` %d is not a multiple of `channels` %d: stream g * channels + c is channel c of group g.",
                   config->num_streams, channels);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const pv_status_t st = pv_koala_batch_init_config(access_key, model_path, device, config, object);
    if (st != PV_STATUS_SUCCESS || channels == 1) return st;
    return kns_api::guarded([&] {
        std::string err;
        if (!(*object)->engine->enable_channels(channels, &err)) {
            pv_koala_batch_delete(*object);
            *object = nullptr;
            push_error(0x65, "%s", err.c_str());
            return PV_STATUS_OUT_OF_MEMORY;
        }
        (*object)->channels = channels;
        return PV_STATUS_SUCCESS;
    });
}

PV_API pv_status_t pv_koala_batch_channels(const pv_koala_batch_t *object, int32_t *channels) {
    kns_api::clear_errors();
    if (!object || !channels) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "channels" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *channels = object->channels;
    return PV_STATUS_SUCCESS;
}
