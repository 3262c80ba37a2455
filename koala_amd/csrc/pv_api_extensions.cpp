// pv_api_extensions.cpp -- the C ABI of the batch handles that are made above pv_koala_batch_init_rate (include/pv_koala_batch.h; DESIGN.md
// section 2, fourth to seventh extension): packet handles (pv_koala_batch_init_packets, _is_packet_handle, _process_packets), sample formats
// and the handles at 44 100 and 22 050 Hz (pv_koala_batch_init_config, _sample_format) and channels (pv_koala_batch_init_channels,
// _channels, _set_channel_link, _get_channel_link) and the high-band carry (_set_high_band, _get_high_band).  Each constructor calls the one below it and then enables its feature on the engine behind the finished handle; the
// processing entry points (pv_api.cpp, and _process_packets here) read the engine and the handle's two own values, sample_rate and
// packet_samples.
#include "pv_api_internal.h"

using kns_api::push_error;

namespace kns_api {

// The last step of such a constructor: `step(&err)` enables a feature on the engine of the finished handle *object.  A step that fails
// -- it returns false, or it throws (a host allocation; guarded() picks the status and the message) -- takes the handle with it: the
// caller gets the status and *object == NULL, never a handle without the feature it asked for.
template <class Step>
static pv_status_t enable_or_delete(pv_koala_batch_t **object, Step &&step) {
    const pv_status_t st = guarded([&] {
        std::string err;
        if (step(&err)) return PV_STATUS_SUCCESS;
        push_error(0x65, "%s", err.c_str());
        return PV_STATUS_OUT_OF_MEMORY;
    });
    if (st != PV_STATUS_SUCCESS) {
        pv_koala_batch_delete(*object);
        *object = nullptr;
    }
    return st;
}

}  // namespace kns_api

using kns_api::enable_or_delete;

// ------------------------------------------------------------------------------------------------ packet handles
// A packet handle is a batch handle (pv_api.cpp) with packet_samples set: the frame entry points refuse it there, the calls below refuse
// a frame handle here.

PV_API pv_status_t pv_koala_batch_init_packets(const char *access_key, const char *model_path, const char *device, int32_t num_streams,
                                               int32_t max_samples_per_call, pv_koala_precision_t precision, int32_t sample_rate,
                                               pv_koala_batch_t **object) {
    kns_api::clear_errors();
    if (max_samples_per_call <= 0) {
        push_error(0x66, "`max_samples_per_call` must be positive.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!kns::rs_rate_ok(sample_rate)) {
        push_error(0x66, "`sample_rate` %d is not one of 8000, 12000, 16000, 24000, 32000, 48000.", sample_rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const int32_t F = kns::rs_frame_length(sample_rate);
    const int32_t max_frames = (int32_t) (((int64_t) max_samples_per_call + F - 1) / F);
    pv_status_t st = pv_koala_batch_init_rate(access_key, model_path, device, num_streams, max_frames, precision, sample_rate, object);
    if (st != PV_STATUS_SUCCESS) return st;
    st = enable_or_delete(object, [&](std::string *err) { return (*object)->engine->enable_packets(max_samples_per_call, err); });
    if (st == PV_STATUS_SUCCESS) (*object)->packet_samples = max_samples_per_call;
    return st;
}

PV_API pv_status_t pv_koala_batch_is_packet_handle(const pv_koala_batch_t *object, int32_t *is_packet_handle) {
    kns_api::clear_errors();
    if (!object || !is_packet_handle) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "is_packet_handle" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *is_packet_handle = object->packet_samples ? 1 : 0;
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_process_packets(pv_koala_batch_t *object, const pv_koala_batch_packets_t *call) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!call) {
        push_error(0x64, "Argument `call` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (call->struct_size != (int32_t) sizeof(pv_koala_batch_packets_t)) {
        push_error(0x66, "`struct_size` %d is not sizeof(pv_koala_batch_packets_t) = %d.", call->struct_size,
                   (int) sizeof(pv_koala_batch_packets_t));
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!object->packet_samples) {
        push_error(0x66, "Packet calls are not available on a frame handle: make the handle with pv_koala_batch_init_packets.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (!call->counts || !call->pcm || !call->enhanced) {
        push_error(0x64, "Argument `%s` is NULL.", !call->counts ? "counts" : call->pcm ? "enhanced" : "pcm");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    kns::PacketCall c{call->max_samples, call->counts, call->pcm, call->enhanced, call->restart, call->report, call->report_frames, call->frames};
    if (kns_api::check_settings(object->settings, object->engine, false) != PV_STATUS_SUCCESS) return PV_STATUS_INVALID_ARGUMENT;
    kns_api::carry(object->settings, &c.opt);
    return kns_api::guarded([&] {
        std::string err;
        const kns::Status status = object->engine->run_packets(c, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : kns_api::engine_failure(status, 0x33D, err);
    });
}

// ------------------------------------------------------------------------------------------------ sample formats, 44 100 and 22 050 Hz
// One struct-taking constructor over the ones above: with PV_KOALA_SAMPLE_S16 the handle is what they return; any other format is set on
// the engine, whose processing entry points then take and deliver elements of that format through the pointers they have always had.

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
    pv_status_t st = pv_koala_batch_init_packets(access_key, model_path, device, config->num_streams, inner_max, precision, kns::kRate16k, object);
    if (st != PV_STATUS_SUCCESS) return st;
    st = enable_or_delete(object, [&](std::string *err) { return (*object)->engine->enable_fractional(rate, max_samples, err); });
    if (st == PV_STATUS_SUCCESS) {
        (*object)->sample_rate = rate;
        (*object)->packet_samples = max_samples;
    }
    return st;
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
    const pv_status_t st =
        kns::fr_rate_ok(config->sample_rate) ? init_fractional(access_key, model_path, device, config, precision, object) :
        config->max_samples_per_call > 0
            ? pv_koala_batch_init_packets(access_key, model_path, device, config->num_streams, config->max_samples_per_call, precision,
                                          config->sample_rate, object)
            : pv_koala_batch_init_rate(access_key, model_path, device, config->num_streams, config->max_frames_per_call, precision,
                                       config->sample_rate, object);
    if (st != PV_STATUS_SUCCESS || config->sample_format == PV_KOALA_SAMPLE_S16) return st;
    return enable_or_delete(object, [&](std::string *err) { return (*object)->engine->set_format(config->sample_format, err); });
}

PV_API pv_status_t pv_koala_batch_sample_format(const pv_koala_batch_t *object, int32_t *sample_format) {
    kns_api::clear_errors();
    if (!object || !sample_format) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "sample_format" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *sample_format = object->engine->sample_format();
    return PV_STATUS_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ channels
// The layout of `pcm` and `enhanced`, set like the sample format and outside it: with channels == 1 the handle is what
// pv_koala_batch_init_config returns; any other count is set on the engine, whose processing entry points then take and deliver
// interleaved group rows.  The config struct does not grow: the count is an argument.

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
    return enable_or_delete(object, [&](std::string *err) { return (*object)->engine->enable_channels(channels, err); });
}

PV_API pv_status_t pv_koala_batch_channels(const pv_koala_batch_t *object, int32_t *channels) {
    kns_api::clear_errors();
    if (!object || !channels) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "channels" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *channels = object->engine->channels();
    return PV_STATUS_SUCCESS;
}

// The link of a handle's channels (eighth extension): a value of the handle that every call carries to the engine, like
// the attenuation limit -- no device work, no wait; the next call is the first to see it.
PV_API pv_status_t pv_koala_batch_set_channel_link(pv_koala_batch_t *object, int32_t link) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (link != PV_KOALA_CHANNEL_LINK_NONE && link != PV_KOALA_CHANNEL_LINK_MAX) {
        push_error(0x66, "`link` %d is not one of PV_KOALA_CHANNEL_LINK_NONE, _MAX (0 ... 1).", link);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    const int channels = object->engine->channels();
    if (link == PV_KOALA_CHANNEL_LINK_MAX && !kns::Engine::channel_link_ok(channels)) {
        push_error(0x66, "PV_KOALA_CHANNEL_LINK_MAX needs a handle whose `channels` is 2, 4 or 8: this handle's `channels` is %d, and a group must "
                         "lie inside one 16-row mask tile.", channels);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    object->settings.link = link;
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_get_channel_link(const pv_koala_batch_t *object, int32_t *link) {
    kns_api::clear_errors();
    if (!object || !link) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "link" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *link = object->settings.link;
    return PV_STATUS_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ high-band carry
// The mode of a handle (ninth extension): a value of the handle that every call carries to the engine, like the link --
// no device work, no wait; the next call is the first to see it.  Turning it on counts an epoch: the engine clears the feature's state when
// it sees a new one, so the high band is that of streams that began with the next call.  Not yet: 24 kHz and 44 100 / 22 050 Hz, packet handles.
PV_API pv_status_t pv_koala_batch_set_high_band(pv_koala_batch_t *object, int32_t mode) {
    kns_api::clear_errors();
    if (!object) {
        push_error(0x64, "Argument `object` is NULL.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (mode != PV_KOALA_HIGH_BAND_NONE && mode != PV_KOALA_HIGH_BAND_CARRY) {
        push_error(0x66, "`mode` %d is not one of PV_KOALA_HIGH_BAND_NONE, _CARRY (0 ... 1).", mode);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (mode == PV_KOALA_HIGH_BAND_CARRY && !kns::hb_rate_ok(object->sample_rate)) {
        push_error(0x66, "PV_KOALA_HIGH_BAND_CARRY needs a handle whose `sample_rate` is 32000 or 48000: this handle's `sample_rate` is %d (16000 and "
                         "below have no band to carry; 24000, 44100 and 22050 are not available yet).", object->sample_rate);
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (mode == PV_KOALA_HIGH_BAND_CARRY && object->packet_samples) {
        push_error(0x66, "PV_KOALA_HIGH_BAND_CARRY is not available yet on a packet handle.");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    if (mode == PV_KOALA_HIGH_BAND_CARRY && !object->settings.high_band) ++object->settings.high_band_epoch;
    object->settings.high_band = mode;
    return PV_STATUS_SUCCESS;
}

PV_API pv_status_t pv_koala_batch_get_high_band(const pv_koala_batch_t *object, int32_t *mode) {
    kns_api::clear_errors();
    if (!object || !mode) {
        push_error(0x64, "Argument `%s` is NULL.", object ? "mode" : "object");
        return PV_STATUS_INVALID_ARGUMENT;
    }
    *mode = object->settings.high_band;
    return PV_STATUS_SUCCESS;
}
