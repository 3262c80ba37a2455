// pv_api_packets.cpp -- the C ABI of packet handles (include/pv_koala_batch.h: pv_koala_batch_init_packets, _is_packet_handle,
// _process_packets; DESIGN.md section 2, fourth extension).  A packet handle is a batch handle (pv_api.cpp) with packet_samples set: the
// frame entry points refuse it there, the calls below refuse a frame handle here.
#include "pv_api_internal.h"

using kns_api::push_error;

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
    return kns_api::guarded([&] {
        std::string err;
        if (!(*object)->engine->enable_packets(max_samples_per_call, &err)) {
            pv_koala_batch_delete(*object);
            *object = nullptr;
            push_error(0x65, "%s", err.c_str());
            return PV_STATUS_OUT_OF_MEMORY;
        }
        (*object)->packet_samples = max_samples_per_call;
        return PV_STATUS_SUCCESS;
    });
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
    if (object->limit.any) {
        c.min_gain = object->limit.gain.data();
        c.min_gain_rev = object->limit.rev;
    }
    return kns_api::guarded([&] {
        std::string err;
        const kns::Status status = object->engine->run_packets(c, &err);
        return status == kns::Status::kOk ? PV_STATUS_SUCCESS : kns_api::engine_failure(status, 0x33D, err);
    });
}

