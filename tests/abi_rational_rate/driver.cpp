// Drives the C ABI at the two rational rates, 12 000 and 24 000 Hz (include/pv_koala_batch.h: pv_koala_batch_init_rate,
// pv_koala_batch_init_packets, and what pv_koala_batch_frame_length / _delay_sample / _state_size answer there) under AddressSanitizer +
// UndefinedBehaviorSanitizer: the constants of DESIGN.md section 2 (third extension, generalised), the refusal text with its six rates,
// the rates that stay refused, and the refusal of asynchronous calls.  Linked with koala_amd/csrc/pv_api*.cpp and the
// host-only engine double of tests/abi_sanitizer (engine_stub.cpp): no GPU, no HIP runtime.  Exit status 0 = every expectation held and
// the sanitizers stayed silent.  usage: driver <model.kns>
#include "../abi_sanitizer/expect.h"

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <model.kns>\n", argv[0]);
        return 2;
    }
    const char *model = argv[1];
    const int B = 3, T = 2;
    std::string msg;
    pv_koala_batch_t *h = nullptr;

    // ---- still refused, by both creators; the text lists the six rates and names the argument
    for (int32_t bad : {0, 16001, 44100, 96000, -12000, 11025, 22050}) {
        EXPECT(pv_koala_batch_init_rate("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, bad, &h) == PV_STATUS_INVALID_ARGUMENT);
        EXPECT(drain(&msg) == 1 && has(msg, "`sample_rate`") && has(msg, "8000, 12000, 16000, 24000, 32000, 48000") && h == nullptr);
        EXPECT(pv_koala_batch_init_packets("k", model, "best", B, 480, PV_KOALA_PRECISION_FP32, bad, &h) == PV_STATUS_INVALID_ARGUMENT);
        EXPECT(drain(&msg) == 1 && has(msg, "`sample_rate`") && has(msg, "8000, 12000, 16000, 24000, 32000, 48000") && h == nullptr);
    }

    // ---- the two rates: frame handles
    const struct {
        int32_t rate, frame, delay, record, packet_delay, packet_record;
    } want[] = {{12000, 192, 240, 10240 + 224, 431, 10240 + 224 + 400}, {24000, 384, 456, 10240 + 240, 839, 10240 + 240 + 784}};
    for (const auto &w : want) {
        h = nullptr;
        EXPECT(pv_koala_batch_init_rate("k", model, "best", B, T, PV_KOALA_PRECISION_BF16, w.rate, &h) == PV_STATUS_SUCCESS && h != nullptr);
        if (!h) continue;
        int32_t v = -1;
        EXPECT(pv_koala_batch_sample_rate(h, &v) == PV_STATUS_SUCCESS && v == w.rate && drain() == 0);
        EXPECT(pv_koala_batch_frame_length(h, &v) == PV_STATUS_SUCCESS && v == w.frame);
        EXPECT(pv_koala_batch_delay_sample(h, &v) == PV_STATUS_SUCCESS && v == w.delay);
        EXPECT(pv_koala_batch_state_size(h, &v) == PV_STATUS_SUCCESS && v == w.record);
        EXPECT(pv_koala_batch_is_packet_handle(h, &v) == PV_STATUS_SUCCESS && v == 0);

        // asynchronous calls are refused with one message and nothing written.  (The engine double moves num_frames * 256 samples per
        // stream whatever the rate, so the buffers are sized for the larger of the two.)
        const size_t n = (size_t) B * T * (w.frame > 256 ? w.frame : 256);
        std::vector<int16_t> in(n), out(n, (int16_t) -7);
        for (size_t i = 0; i < n; ++i) in[i] = (int16_t) (i * 29);
        std::vector<uint8_t> reset((size_t) B * T, 0);
        pv_koala_batch_call_t call;
        memset(&call, 0, sizeof(call));
        call.struct_size = (int32_t) sizeof(call);
        call.num_frames = T;
        call.pcm = in.data();
        call.enhanced = out.data();
        call.asynchronous = 1;
        EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, "synchronous") && has(msg, std::to_string(w.rate).c_str()));
        EXPECT(pv_koala_batch_process_chunk_resets_async(h, T, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT &&
               drain(&msg) == 1 && has(msg, "synchronous"));
        EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "synchronous"));
        for (int16_t o : out) EXPECT(o == -7);
        // the synchronous forms are taken
        call.asynchronous = 0;
        EXPECT(pv_koala_batch_process_chunk(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_chunk_resets(h, T, in.data(), out.data(), reset.data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_SUCCESS && drain() == 0);
        // a record buffer of exactly state_size bytes per stream: a write past it is the sanitizer's to find
        std::vector<uint8_t> records((size_t) B * w.record);
        EXPECT(pv_koala_batch_export_state(h, B, nullptr, records.data()) == PV_STATUS_SUCCESS);
        pv_koala_batch_delete(h);

        // ---- a packet handle at the rate: F - 1 samples of lead on top, and the version-3 tail (uint32 fill, int16[F - 1], padded to 16)
        h = nullptr;
        EXPECT(pv_koala_batch_init_packets("k", model, "best", B, w.rate / 50, PV_KOALA_PRECISION_FP32, w.rate, &h) == PV_STATUS_SUCCESS &&
               h != nullptr);
        if (!h) continue;
        EXPECT(pv_koala_batch_is_packet_handle(h, &v) == PV_STATUS_SUCCESS && v == 1);
        EXPECT(pv_koala_batch_sample_rate(h, &v) == PV_STATUS_SUCCESS && v == w.rate);
        EXPECT(pv_koala_batch_frame_length(h, &v) == PV_STATUS_SUCCESS && v == w.frame);
        EXPECT(pv_koala_batch_delay_sample(h, &v) == PV_STATUS_SUCCESS && v == w.packet_delay && v == w.delay + w.frame - 1);
        EXPECT(pv_koala_batch_state_size(h, &v) == PV_STATUS_SUCCESS && v == w.packet_record);
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1);
        pv_koala_batch_delete(h);
    }
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}
