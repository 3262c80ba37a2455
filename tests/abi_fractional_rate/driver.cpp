// Drives the C ABI at 44 100 and 22 050 Hz (include/pv_koala_batch.h: pv_koala_batch_init_config with max_samples_per_call > 0) under
// AddressSanitizer + UndefinedBehaviorSanitizer: the one constructor that reaches the two rates and the ones that keep refusing them, the
// queries (sample_rate, delay_sample 1541 / 771, is_packet_handle, sample_format; frame_length refused), and every refusal -- frame and
// asynchronous entry points, stream records, 11 025 Hz -- with exactly one message and nothing processed.  Linked with
// koala_amd/csrc/pv_api*.cpp and the host-only engine double of tests/abi_sanitizer (engine_stub.cpp, whose g_packet_calls counts the
// packet calls that reached it): no GPU, no HIP runtime.  Exit status 0 = every expectation held and the sanitizers stayed silent.
// usage: driver <model.kns>
#include "../abi_sanitizer/expect.h"

extern int g_packet_calls;  // engine_stub.cpp

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <model.kns>\n", argv[0]);
        return 2;
    }
    const char *model = argv[1];
    const int B = 3, N = 1000;
    std::string msg;
    pv_koala_batch_t *h = nullptr;

    const struct {
        int32_t rate, delay;
    } want[] = {{44100, 1541}, {22050, 771}};
    for (const auto &w : want) {
        // ---- the older constructors keep refusing the rate, with their text
        h = nullptr;
        EXPECT(pv_koala_batch_init_rate("k", model, "best", B, 2, PV_KOALA_PRECISION_FP32, w.rate, &h) == PV_STATUS_INVALID_ARGUMENT);
        EXPECT(drain(&msg) == 1 && has(msg, "`sample_rate`") && has(msg, "8000, 12000, 16000, 24000, 32000, 48000") && h == nullptr);
        EXPECT(pv_koala_batch_init_packets("k", model, "best", B, N, PV_KOALA_PRECISION_FP32, w.rate, &h) == PV_STATUS_INVALID_ARGUMENT);
        EXPECT(drain(&msg) == 1 && has(msg, "`sample_rate`") && has(msg, "8000, 12000, 16000, 24000, 32000, 48000") && h == nullptr);
        // ---- init_config without max_samples_per_call: refused, names sample_rate and says "packet handle"
        pv_koala_batch_config_t c = config(B, 2, 0, w.rate, PV_KOALA_SAMPLE_S16);
        EXPECT(pv_koala_batch_init_config("k", model, "best", &c, &h) == PV_STATUS_INVALID_ARGUMENT);
        EXPECT(drain(&msg) == 1 && has(msg, "`sample_rate`") && has(msg, "packet handle") && has(msg, std::to_string(w.rate).c_str()) && h == nullptr);
        c = config(B, 2, (1 << 22) + 1, w.rate, PV_KOALA_SAMPLE_S16);
        EXPECT(pv_koala_batch_init_config("k", model, "best", &c, &h) == PV_STATUS_INVALID_ARGUMENT);
        EXPECT(drain(&msg) == 1 && has(msg, "`max_samples_per_call`") && h == nullptr);

        // ---- the handle, in two formats
        for (pv_koala_sample_format_t fmt : {PV_KOALA_SAMPLE_S16, PV_KOALA_SAMPLE_ULAW}) {
            c = config(B, 0, N, w.rate, fmt);
            h = nullptr;
            EXPECT(pv_koala_batch_init_config("k", model, "best", &c, &h) == PV_STATUS_SUCCESS && h != nullptr && drain() == 0);
            if (!h) continue;
            int32_t v = -1;
            EXPECT(pv_koala_batch_sample_rate(h, &v) == PV_STATUS_SUCCESS && v == w.rate);
            EXPECT(pv_koala_batch_delay_sample(h, &v) == PV_STATUS_SUCCESS && v == w.delay);
            EXPECT(pv_koala_batch_is_packet_handle(h, &v) == PV_STATUS_SUCCESS && v == 1);
            EXPECT(pv_koala_batch_sample_format(h, &v) == PV_STATUS_SUCCESS && v == (int32_t) fmt);
            EXPECT(pv_koala_batch_num_streams(h, &v) == PV_STATUS_SUCCESS && v == B && drain() == 0);
            v = -5;
            EXPECT(pv_koala_batch_frame_length(h, &v) == PV_STATUS_INVALID_ARGUMENT && v == -5 && drain(&msg) == 1 && has(msg, "frame length") &&
                   has(msg, std::to_string(w.rate).c_str()));

            // every refusal: one message, nothing processed, nothing written
            const int before = g_packet_calls;
            std::vector<int16_t> in((size_t) B * N), out((size_t) B * N, (int16_t) -7);
            for (size_t i = 0; i < in.size(); ++i) in[i] = (int16_t) (i * 29);
            std::vector<uint8_t> reset((size_t) B, 0), records(1 << 16, 0xee);
            pv_koala_batch_call_t call;
            memset(&call, 0, sizeof(call));
            call.struct_size = (int32_t) sizeof(call);
            call.num_frames = 1, call.pcm = in.data(), call.enhanced = out.data();
            EXPECT(pv_koala_batch_process(h, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "packet handle"));
            EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "packet handle"));
            EXPECT(pv_koala_batch_process_chunk_resets(h, 1, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
            EXPECT(pv_koala_batch_process_chunk_hold(h, 1, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
            EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
            EXPECT(pv_koala_batch_process_chunk_async(h, 1, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "packet handle"));
            EXPECT(pv_koala_batch_process_chunk_resets_async(h, 1, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
            call.asynchronous = 1;
            EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
            v = -5;
            EXPECT(pv_koala_batch_state_size(h, &v) == PV_STATUS_INVALID_ARGUMENT && v == -5 && drain(&msg) == 1 && has(msg, "records") &&
                   has(msg, std::to_string(w.rate).c_str()));
            EXPECT(pv_koala_batch_export_state(h, B, nullptr, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "records"));
            EXPECT(pv_koala_batch_import_state(h, B, nullptr, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "records"));
            for (uint8_t r : records) EXPECT(r == 0xee);
            for (int16_t o : out) EXPECT(o == -7);
            EXPECT(g_packet_calls == before);

            // a packet call is taken: max_samples up to the CALLER's N (the inner handle's is smaller), counts ragged, zero included
            if (fmt == PV_KOALA_SAMPLE_S16) {
                int32_t counts[B] = {N, 0, 441}, frames[B] = {-1, -1, -1};
                pv_koala_batch_packets_t p;
                memset(&p, 0, sizeof(p));
                p.struct_size = (int32_t) sizeof(p);
                p.max_samples = N, p.counts = counts, p.pcm = in.data(), p.enhanced = out.data(), p.frames = frames;
                EXPECT(pv_koala_batch_process_packets(h, &p) == PV_STATUS_SUCCESS && drain() == 0 && g_packet_calls == before + 1);
                EXPECT(out[0] == in[0] && out[N - 1] == in[N - 1] && out[N] == -7 && out[2 * N + 440] == in[2 * N + 440] && out[2 * N + 441] == -7);
            }
            EXPECT(pv_koala_batch_reset(h, nullptr) == PV_STATUS_SUCCESS && pv_koala_batch_reset(h, reset.data()) == PV_STATUS_SUCCESS);
            pv_koala_batch_delete(h);
        }
    }

    // ---- 11 025 Hz: not yet, by name; other rates: the text they have always had; the six older rates still come through init_config
    h = nullptr;
    pv_koala_batch_config_t c = config(B, 0, N, 11025, PV_KOALA_SAMPLE_S16);
    EXPECT(pv_koala_batch_init_config("k", model, "best", &c, &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`sample_rate`") &&
           has(msg, "11025") && has(msg, "not available yet") && h == nullptr);
    c = config(B, 0, N, 96000, PV_KOALA_SAMPLE_S16);
    EXPECT(pv_koala_batch_init_config("k", model, "best", &c, &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`sample_rate`") && h == nullptr);
    c = config(B, 0, 960, 48000, PV_KOALA_SAMPLE_S16);
    EXPECT(pv_koala_batch_init_config("k", model, "best", &c, &h) == PV_STATUS_SUCCESS && h != nullptr);
    if (h) {
        int32_t v = -1;
        EXPECT(pv_koala_batch_frame_length(h, &v) == PV_STATUS_SUCCESS && v == 768);
        EXPECT(pv_koala_batch_delay_sample(h, &v) == PV_STATUS_SUCCESS && v == 768 + 144 + 767);
        EXPECT(pv_koala_batch_state_size(h, &v) == PV_STATUS_SUCCESS && v == 10240 + 384 + 1552);
        pv_koala_batch_delete(h);
    }
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}
