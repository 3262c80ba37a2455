// Drives the sample-rate entry points of the C ABI (include/pv_koala_batch.h: pv_koala_batch_init_rate, pv_koala_batch_sample_rate,
// pv_koala_batch_frame_length, and what pv_koala_batch_delay_sample / pv_koala_batch_state_size answer for a handle's rate) under
// AddressSanitizer + UndefinedBehaviorSanitizer: NULL arguments, refused rates, the four rates' frame lengths, delays and record sizes, and
// the refusal of asynchronous calls on a handle that is not at 16 kHz.  Linked with koala_amd/csrc/pv_api.cpp and the host-only engine
// double of tests/abi_sanitizer (engine_stub.cpp): no GPU, no HIP runtime.  Exit status 0 = every expectation held and the sanitizers
// stayed silent.  usage: driver <model.kns>
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

    // ---- refused at creation: NULL arguments as for pv_koala_batch_init, rates outside the four; no handle is made
    EXPECT(pv_koala_batch_init_rate("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, 8000, nullptr) == PV_STATUS_INVALID_ARGUMENT &&
           drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_init_rate(nullptr, model, "best", B, T, PV_KOALA_PRECISION_FP32, 8000, &h) == PV_STATUS_INVALID_ARGUMENT &&
           drain(&msg) == 1 && has(msg, "`access_key`") && h == nullptr);
    EXPECT(pv_koala_batch_init_rate("k", nullptr, "best", B, T, PV_KOALA_PRECISION_FP32, 8000, &h) == PV_STATUS_INVALID_ARGUMENT &&
           drain(&msg) == 1 && has(msg, "`model_path`") && h == nullptr);
    for (int32_t bad : {0, 16001, 44100, -8000, 96000}) {
        EXPECT(pv_koala_batch_init_rate("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, bad, &h) == PV_STATUS_INVALID_ARGUMENT);
        EXPECT(drain(&msg) == 1 && has(msg, "`sample_rate`") && h == nullptr);
    }

    // ---- the four rates
    const struct {
        int32_t rate, frame, delay, record;
    } want[] = {{8000, 128, 176, 10240 + 288}, {16000, 256, 256, 10240}, {32000, 512, 608, 10240 + 288}, {48000, 768, 912, 10240 + 384}};
    for (const auto &w : want) {
        h = nullptr;
        EXPECT(pv_koala_batch_init_rate("k", model, "best", B, T, PV_KOALA_PRECISION_BF16, w.rate, &h) == PV_STATUS_SUCCESS && h != nullptr);
        if (!h) continue;
        int32_t v = -1;
        EXPECT(pv_koala_batch_sample_rate(h, &v) == PV_STATUS_SUCCESS && v == w.rate && drain() == 0);
        EXPECT(pv_koala_batch_frame_length(h, &v) == PV_STATUS_SUCCESS && v == w.frame);
        EXPECT(pv_koala_batch_delay_sample(h, &v) == PV_STATUS_SUCCESS && v == w.delay);
        EXPECT(pv_koala_batch_state_size(h, &v) == PV_STATUS_SUCCESS && v == w.record);
        EXPECT(pv_koala_batch_num_streams(h, &v) == PV_STATUS_SUCCESS && v == B);
        v = -5;
        EXPECT(pv_koala_batch_sample_rate(nullptr, &v) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
        EXPECT(pv_koala_batch_sample_rate(h, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`sample_rate`"));
        EXPECT(pv_koala_batch_frame_length(nullptr, &v) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
        EXPECT(pv_koala_batch_frame_length(h, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`frame_length`"));
        EXPECT(v == -5);

        // asynchronous calls: taken at 16 kHz, refused elsewhere with one message and nothing written.  (The engine double moves
        // num_frames * 256 samples per stream whatever the rate, so the buffers are sized for the larger of the two.)
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
        if (w.rate == 16000) {
            EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS);
            EXPECT(pv_koala_batch_process_chunk_resets_async(h, T, in.data(), out.data(), reset.data()) == PV_STATUS_SUCCESS);
            EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_SUCCESS && drain() == 0);
        } else {
            EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
                   has(msg, "synchronous"));
            EXPECT(pv_koala_batch_process_chunk_resets_async(h, T, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT &&
                   drain(&msg) == 1 && has(msg, "synchronous"));
            EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "synchronous"));
            for (int16_t o : out) EXPECT(o == -7);
        }
        EXPECT(pv_koala_batch_async_wait(h, 0) == PV_STATUS_SUCCESS);
        // the synchronous forms are taken at every rate
        call.asynchronous = 0;
        EXPECT(pv_koala_batch_process_chunk(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_chunk_resets(h, T, in.data(), out.data(), reset.data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_SUCCESS && drain() == 0);
        // a record buffer of exactly state_size bytes per stream: a write past it is the sanitizer's to find
        std::vector<uint8_t> records((size_t) B * w.record);
        EXPECT(pv_koala_batch_export_state(h, B, nullptr, records.data()) == PV_STATUS_SUCCESS);
        pv_koala_batch_delete(h);
    }

    // pv_koala_batch_init is the 16 kHz handle
    h = nullptr;
    EXPECT(pv_koala_batch_init("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, &h) == PV_STATUS_SUCCESS && h != nullptr);
    int32_t v = -1;
    EXPECT(pv_koala_batch_sample_rate(h, &v) == PV_STATUS_SUCCESS && v == 16000);
    EXPECT(pv_koala_batch_frame_length(h, &v) == PV_STATUS_SUCCESS && v == 256);
    EXPECT(pv_koala_batch_delay_sample(h, &v) == PV_STATUS_SUCCESS && v == 256);
    pv_koala_batch_delete(h);
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}
