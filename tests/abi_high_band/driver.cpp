// Drives the high-band entry points of the C ABI (include/pv_koala_batch.h: pv_koala_batch_set_high_band / get_high_band) and the refusals
// that hold while the carry is on, under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU.  Linked with koala_amd/csrc/pv_api*.cpp
// and a RECORDING copy of the host-only engine double: tests/test_high_band_abi.py writes it from tests/abi_sanitizer/engine_stub.cpp (left as
// it is) with tests/test_channel_link_abi.recording_double, which keeps the kns::Call that reaches Engine::process.  Exit status 0 = every
// expectation held.  usage: driver <model.kns>
#include "../abi_sanitizer/expect.h"
#include "kns_engine.h"

namespace kns {
extern Call g_seen_call;
extern int g_seen_calls;
}  // namespace kns

static pv_koala_batch_t *open_handle(const char *model, int B, int frames, int samples, int rate) {
    pv_koala_batch_t *h = nullptr;
    pv_koala_batch_config_t c = config(B, frames, samples, rate, PV_KOALA_SAMPLE_S16);
    EXPECT(pv_koala_batch_init_config("k", model, "best", &c, &h) == PV_STATUS_SUCCESS && h != nullptr);
    return h;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <model.kns>\n", argv[0]);
        return 2;
    }
    const int B = 4, T = 3;
    std::string msg;
    int32_t v = -7;

    // ---- NULL objects and out-pointers
    EXPECT(pv_koala_batch_set_high_band(nullptr, PV_KOALA_HIGH_BAND_CARRY) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_set_high_band(nullptr, PV_KOALA_HIGH_BAND_NONE) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_get_high_band(nullptr, &v) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`") && v == -7);
    EXPECT(pv_koala_batch_get_high_band(nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));

    // ---- NONE everywhere; CARRY refused by rate (the message names sample_rate) and on packet handles
    const int rates[] = {8000, 12000, 16000, 24000, 32000, 48000};
    for (int rate : rates) {
        pv_koala_batch_t *h = open_handle(argv[1], B, T, 0, rate);
        if (!h) continue;
        EXPECT(pv_koala_batch_get_high_band(h, &v) == PV_STATUS_SUCCESS && v == PV_KOALA_HIGH_BAND_NONE && drain() == 0);
        EXPECT(pv_koala_batch_get_high_band(h, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`mode`"));
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_NONE) == PV_STATUS_SUCCESS && drain() == 0);
        for (int bad : {-1, 2, 1 << 30}) {
            EXPECT(pv_koala_batch_set_high_band(h, bad) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`mode`"));
        }
        const bool ok = rate == 32000 || rate == 48000;
        const pv_status_t st = pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_CARRY);
        if (ok) {
            EXPECT(st == PV_STATUS_SUCCESS && drain() == 0);
        } else {
            EXPECT(st == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`sample_rate`") && has(msg, std::to_string(rate).c_str()));
        }
        EXPECT(pv_koala_batch_get_high_band(h, &v) == PV_STATUS_SUCCESS && v == (ok ? 1 : 0));
        EXPECT(pv_koala_batch_set_high_band(h, 7) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);  // a refused change leaves the setting
        EXPECT(pv_koala_batch_get_high_band(h, &v) == PV_STATUS_SUCCESS && v == (ok ? 1 : 0));
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_NONE) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_get_high_band(h, &v) == PV_STATUS_SUCCESS && v == 0);
        pv_koala_batch_delete(h);
    }
    for (int rate : {16000, 48000, 44100, 22050}) {  // packet handles, the fractional rates among them
        pv_koala_batch_t *h = open_handle(argv[1], B, 0, 960, rate);
        if (!h) continue;
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_NONE) == PV_STATUS_SUCCESS && drain() == 0);
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_CARRY) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, rate == 48000 ? "packet handle" : "`sample_rate`"));
        EXPECT(pv_koala_batch_get_high_band(h, &v) == PV_STATUS_SUCCESS && v == 0);
        pv_koala_batch_delete(h);
    }

    // ---- the setting and its epoch travel in the Call; what the carry refuses reaches the engine zero times
    pv_koala_batch_t *h = open_handle(argv[1], B, T, 0, 48000);
    if (h) {
        const size_t n = (size_t) B * T * 768;
        std::vector<int16_t> in(n, 3), out(n, 0x1111);
        std::vector<uint8_t> hold(B, 0), reset((size_t) B * T, 0);
        std::vector<float> rep((size_t) B * T * 4, -1.0f);
        std::vector<uint8_t> records;
        int32_t size = -7;
        EXPECT(pv_koala_batch_state_size(h, &size) == PV_STATUS_SUCCESS && size > 0);
        records.assign((size_t) B * size, 0);
        auto frame_call = [&](int which, pv_status_t want) {
            const int before = kns::g_seen_calls;
            pv_status_t st = PV_STATUS_RUNTIME_ERROR;
            if (which == 0) st = pv_koala_batch_process_chunk(h, T, in.data(), out.data());
            if (which == 1) st = pv_koala_batch_process_chunk_resets(h, T, in.data(), out.data(), reset.data());
            if (which == 2) st = pv_koala_batch_process_chunk_hold(h, T, in.data(), out.data(), hold.data());
            if (which == 3) {
                pv_koala_batch_call_t call;
                memset(&call, 0, sizeof(call));
                call.struct_size = (int32_t) sizeof(call);
                call.num_frames = T, call.pcm = in.data(), call.enhanced = out.data(), call.reset = reset.data(), call.hold = hold.data();
                call.report = rep.data();
                st = pv_koala_batch_process_call(h, &call);
            }
            EXPECT(st == want && kns::g_seen_calls == before + (want == PV_STATUS_SUCCESS ? 1 : 0));
        };
        for (int w = 0; w < 4; ++w) {  // off: the plain call
            frame_call(w, PV_STATUS_SUCCESS);
            EXPECT(kns::g_seen_call.high_band == 0);
        }
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_CARRY) == PV_STATUS_SUCCESS);
        unsigned epoch = 0;
        for (int w = 0; w < 4; ++w) {  // on: all-zero masks are the plain masks, a frame-0 reset is taken
            reset[(size_t) 1 * T] = w == 1 || w == 3;
            frame_call(w, PV_STATUS_SUCCESS);
            EXPECT(kns::g_seen_call.high_band == 1 && (w == 0 || kns::g_seen_call.high_band_epoch == epoch));
            epoch = kns::g_seen_call.high_band_epoch;
        }
        reset[(size_t) 1 * T] = 0;
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_CARRY) == PV_STATUS_SUCCESS);  // on while on: the same epoch, nothing is cleared
        frame_call(0, PV_STATUS_SUCCESS);
        EXPECT(kns::g_seen_call.high_band == 1 && kns::g_seen_call.high_band_epoch == epoch);
        // refused by name, before the engine
        std::fill(out.begin(), out.end(), (int16_t) 0x1111);
        hold[2] = 1;
        for (int w : {2, 3}) {
            frame_call(w, PV_STATUS_INVALID_ARGUMENT);
            EXPECT(drain(&msg) == 1 && has(msg, "`hold[2]`") && has(msg, "high-band"));
        }
        hold[2] = 0;
        reset[(size_t) 3 * T + 2] = 1;
        for (int w : {1, 3}) {
            frame_call(w, PV_STATUS_INVALID_ARGUMENT);
            EXPECT(drain(&msg) == 1 && has(msg, "`reset[3][2]`") && has(msg, "high-band"));
        }
        reset[(size_t) 3 * T + 2] = 0;
        for (int16_t s : out) {
            if (s != 0x1111) {
                EXPECT(!"a refused call wrote `enhanced`");
                break;
            }
        }
        size = -7;
        EXPECT(pv_koala_batch_state_size(h, &size) == PV_STATUS_INVALID_ARGUMENT && size == -7 && drain(&msg) == 1 && has(msg, "state_size") && has(msg, "high-band"));
        EXPECT(pv_koala_batch_export_state(h, B, nullptr, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "export_state") && has(msg, "high-band"));
        EXPECT(pv_koala_batch_import_state(h, B, nullptr, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "import_state") && has(msg, "high-band"));
        // the asynchronous entry points stay refused at this rate, carry or not
        EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "Asynchronous"));
        // off and on again: the plain call, then a new epoch
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_NONE) == PV_STATUS_SUCCESS);
        hold[2] = 1;
        frame_call(2, PV_STATUS_SUCCESS);
        hold[2] = 0;
        EXPECT(kns::g_seen_call.high_band == 0);
        EXPECT(pv_koala_batch_state_size(h, &size) == PV_STATUS_SUCCESS && size > 0);
        EXPECT(pv_koala_batch_export_state(h, B, nullptr, records.data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_CARRY) == PV_STATUS_SUCCESS);
        frame_call(0, PV_STATUS_SUCCESS);
        EXPECT(kns::g_seen_call.high_band == 1 && kns::g_seen_call.high_band_epoch != epoch);
        EXPECT(pv_koala_batch_reset(h, nullptr) == PV_STATUS_SUCCESS);  // a reset keeps the setting
        EXPECT(pv_koala_batch_get_high_band(h, &v) == PV_STATUS_SUCCESS && v == 1);
        pv_koala_batch_delete(h);
    }
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}
