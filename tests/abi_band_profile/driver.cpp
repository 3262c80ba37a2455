// Drives the band-profile entry points of the C ABI (include/pv_koala_batch.h: pv_koala_batch_set_band_profile / get_band_profile,
// pv_koala_set_band_profile / get_band_profile) under AddressSanitizer + UndefinedBehaviorSanitizer: table validation, "a refused call
// changes nothing", the revision's table across changes, and the profile interleaved with calls, resets and handle deletion.  Linked with
// koala_amd/csrc/pv_api*.cpp and the host-only engine double of tests/abi_sanitizer (engine_stub.cpp): no GPU, no HIP runtime.
// Exit status 0 = every expectation held and the sanitizers stayed silent.  usage: driver <model.kns>
#include <math.h>

#include <limits>

#include "../abi_sanitizer/expect.h"

static const int K = PV_KOALA_NUM_BINS;

static void batch(const char *model) {
    const int B = 5, T = 2;
    pv_koala_batch_t *h = nullptr;
    EXPECT(pv_koala_batch_init("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, &h) == PV_STATUS_SUCCESS && h != nullptr);
    std::string msg;
    // exactly B x 257 floats each: a read or write past the end is the sanitizer's to find
    std::vector<float> lo((size_t) B * K), hi((size_t) B * K), want_lo((size_t) B * K, 0.0f), want_hi((size_t) B * K, 1.0f), a(K), b(K);
    std::vector<int32_t> idx(B);
    auto same = [&] {
        for (int s = 0; s < B; ++s) {
            std::fill(a.begin(), a.end(), -1.0f);
            std::fill(b.begin(), b.end(), -1.0f);
            if (pv_koala_batch_get_band_profile(h, s, a.data(), b.data()) != PV_STATUS_SUCCESS || drain() != 0) return false;
            if (memcmp(a.data(), &want_lo[(size_t) s * K], K * 4) || memcmp(b.data(), &want_hi[(size_t) s * K], K * 4)) return false;
        }
        return true;
    };
    auto fill = [&] {
        for (int s = 0; s < B; ++s)
            for (int k = 0; k < K; ++k) {
                lo[(size_t) s * K + k] = (float) ((s * 7 + k) % 11) / 32.0f;
                hi[(size_t) s * K + k] = lo[(size_t) s * K + k] + (float) ((s + k) % 5) / 8.0f;
            }
    };
    EXPECT(same());  // a new handle: the neutral profile

    // ---- refused: status, one message, nothing changed
    fill();
    EXPECT(pv_koala_batch_set_band_profile(nullptr, B, nullptr, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_get_band_profile(nullptr, 0, a.data(), b.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    for (int32_t bad : {-1, B, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()})
        EXPECT(pv_koala_batch_get_band_profile(h, bad, a.data(), b.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`stream`"));
    for (int32_t count : {0, -1, B + 1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()})
        EXPECT(pv_koala_batch_set_band_profile(h, count, nullptr, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`count`"));
    for (int32_t bad : {-1, B, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()}) {
        for (int i = 0; i < B; ++i) idx[i] = i;
        idx[3] = bad;
        EXPECT(pv_koala_batch_set_band_profile(h, B, idx.data(), lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`streams[3]`"));
        EXPECT(same());
    }
    for (int i = 0; i < B; ++i) idx[i] = i;
    idx[4] = 1;  // slot 1 twice; the entries in front of it are valid and must not have been applied
    EXPECT(pv_koala_batch_set_band_profile(h, B, idx.data(), lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "listed twice"));
    EXPECT(same());
    const float bad_values[] = {nanf(""), -nanf(""), 1.0000001f, -1e-30f, 2.0f, -1.0f, INFINITY, -INFINITY};
    for (float bad : bad_values) {
        fill();
        lo[(size_t) 3 * K + 17] = bad;
        EXPECT(pv_koala_batch_set_band_profile(h, B, nullptr, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, "profile 3, bin 17:") && has(msg, "floor"));
        EXPECT(same());
        fill();
        hi[(size_t) 4 * K + 256] = bad;
        EXPECT(pv_koala_batch_set_band_profile(h, B, nullptr, nullptr, hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, "profile 4, bin 256:") && has(msg, "ceiling"));
        EXPECT(same());
    }
    fill();
    lo[(size_t) 2 * K] = 0.75f, hi[(size_t) 2 * K] = 0.5f;  // floor above ceiling, bin 0 of entry 2
    EXPECT(pv_koala_batch_set_band_profile(h, B, nullptr, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
           has(msg, "profile 2, bin 0:") && has(msg, "above"));
    EXPECT(same());
    // (a floor alone above the implied ceiling of 1 cannot be: it is outside [0, 1]; a ceiling alone below the implied floor of 0 neither)

    // ---- accepted: all slots, a list in any order, NULL curves, -0
    fill();
    want_lo = lo, want_hi = hi;
    EXPECT(pv_koala_batch_set_band_profile(h, B, nullptr, lo.data(), hi.data()) == PV_STATUS_SUCCESS && drain() == 0 && same());
    const int32_t some[2] = {4, 1};
    std::vector<float> two((size_t) 2 * K, 0.25f);
    two[5] = -0.0f;
    EXPECT(pv_koala_batch_set_band_profile(h, 2, some, two.data(), nullptr) == PV_STATUS_SUCCESS);  // ceiling NULL: ones
    for (int k = 0; k < K; ++k) {
        want_lo[(size_t) 4 * K + k] = k == 5 ? 0.0f : 0.25f, want_hi[(size_t) 4 * K + k] = 1.0f;
        want_lo[(size_t) 1 * K + k] = 0.25f, want_hi[(size_t) 1 * K + k] = 1.0f;
    }
    EXPECT(same());  // (memcmp: the -0 came back as +0)
    EXPECT(pv_koala_batch_get_band_profile(h, 0, nullptr, nullptr) == PV_STATUS_SUCCESS && drain() == 0);  // either out-pointer may be NULL
    EXPECT(pv_koala_batch_set_band_profile(h, 1, nullptr, nullptr, nullptr) == PV_STATUS_SUCCESS);  // both NULL: slot 0 neutral again
    for (int k = 0; k < K; ++k) want_lo[k] = 0.0f, want_hi[k] = 1.0f;
    EXPECT(same());

    // ---- interleaved with everything that advances, resets or holds streams: configuration, nothing touches it
    std::vector<int16_t> in((size_t) B * T * 256), out((size_t) B * T * 256);
    for (size_t i = 0; i < in.size(); ++i) in[i] = (int16_t) (i * 31);
    std::vector<uint8_t> reset((size_t) B * T, 0), hold(B, 0), mask(B, 0);
    reset[1] = reset[B * T - 1] = 1, hold[2] = 1, mask[3] = 1;
    EXPECT(pv_koala_batch_process_chunk(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS && same());
    EXPECT(pv_koala_batch_process_chunk_resets(h, T, in.data(), out.data(), reset.data()) == PV_STATUS_SUCCESS && same());
    EXPECT(pv_koala_batch_process_chunk_hold(h, T, in.data(), out.data(), hold.data()) == PV_STATUS_SUCCESS && same());
    EXPECT(pv_koala_batch_reset(h, mask.data()) == PV_STATUS_SUCCESS && same());
    EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS);
    fill();
    want_lo = lo, want_hi = hi;
    EXPECT(pv_koala_batch_set_band_profile(h, B, nullptr, lo.data(), hi.data()) == PV_STATUS_SUCCESS);  // while a call is in flight
    lo[7] = 9.0f;
    EXPECT(pv_koala_batch_set_band_profile(h, B, nullptr, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_batch_async_wait(h, 0) == PV_STATUS_SUCCESS && pv_koala_batch_synchronize(h) == PV_STATUS_SUCCESS && same());
    setenv("STUB_FAIL_PROCESS", "1", 1);
    EXPECT(pv_koala_batch_process_chunk(h, T, in.data(), out.data()) == PV_STATUS_RUNTIME_ERROR && drain() == 2 && same());
    unsetenv("STUB_FAIL_PROCESS");
    int32_t bytes0 = 0;
    EXPECT(pv_koala_batch_state_size(h, &bytes0) == PV_STATUS_SUCCESS && bytes0 > 0);
    pv_koala_batch_delete(h);  // (with a profile in force: the handle's table goes with it -- the leak check's to confirm)
}

// the two "not yet" refusals: a profile that is not neutral with the channel link on, and with the high-band carry on
static void refusals(const char *model) {
    std::string msg;
    std::vector<float> hp(K, 1.0f);
    hp[0] = hp[1] = 0.0f;
    {
        pv_koala_batch_config_t cfg = {};
        cfg.struct_size = (int32_t) sizeof(cfg);
        cfg.num_streams = 4, cfg.max_frames_per_call = 1, cfg.precision = PV_KOALA_PRECISION_FP32, cfg.sample_rate = 16000;
        pv_koala_batch_t *h = nullptr;
        EXPECT(pv_koala_batch_init_channels("k", model, "best", &cfg, 2, &h) == PV_STATUS_SUCCESS && h != nullptr);
        if (!h) return;
        std::vector<int16_t> in(4 * 256, 3), out(4 * 256, 0x5A5A);
        EXPECT(pv_koala_batch_set_channel_link(h, PV_KOALA_CHANNEL_LINK_MAX) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_set_band_profile(h, 1, nullptr, nullptr, hp.data()) == PV_STATUS_SUCCESS);  // setting it is configuration: accepted
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, "band profile") && has(msg, "channel link"));
        for (int16_t v : out) EXPECT(v == 0x5A5A);
        EXPECT(pv_koala_batch_set_band_profile(h, 1, nullptr, nullptr, nullptr) == PV_STATUS_SUCCESS);  // neutral again: the link alone
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_SUCCESS && drain() == 0);
        pv_koala_batch_delete(h);
    }
    {
        pv_koala_batch_t *h = nullptr;
        EXPECT(pv_koala_batch_init_rate("k", model, "best", 2, 1, PV_KOALA_PRECISION_FP32, 48000, &h) == PV_STATUS_SUCCESS && h != nullptr);
        if (!h) return;
        std::vector<int16_t> in(2 * 768, 3), out(2 * 768, 0x5A5A);
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_CARRY) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_set_band_profile(h, 2, nullptr, nullptr, std::vector<float>((size_t) 2 * K, 0.5f).data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, "band profile") && has(msg, "high-band carry"));
        for (int16_t v : out) EXPECT(v == 0x5A5A);
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_NONE) == PV_STATUS_SUCCESS);  // the carry off: the profile alone
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_SUCCESS && drain() == 0);
        pv_koala_batch_delete(h);
    }
}

static void single_stream(const char *model) {
    pv_koala_t *h = nullptr;
    EXPECT(pv_koala_init("k", model, "best", &h) == PV_STATUS_SUCCESS && h != nullptr);
    std::string msg;
    std::vector<float> lo(K, 0.125f), hi(K, 0.5f), a(K, -1.0f), b(K, -1.0f);
    EXPECT(pv_koala_get_band_profile(h, a.data(), b.data()) == PV_STATUS_SUCCESS && a[0] == 0.0f && a[K - 1] == 0.0f && b[0] == 1.0f && b[K - 1] == 1.0f);
    EXPECT(pv_koala_set_band_profile(nullptr, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_get_band_profile(nullptr, a.data(), b.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    lo[200] = nanf("");
    EXPECT(pv_koala_set_band_profile(h, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "profile 0, bin 200:"));
    lo[200] = 0.75f;
    EXPECT(pv_koala_set_band_profile(h, lo.data(), hi.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "profile 0, bin 200:"));
    EXPECT(pv_koala_get_band_profile(h, a.data(), b.data()) == PV_STATUS_SUCCESS && a[200] == 0.0f && b[200] == 1.0f);
    lo[200] = 0.125f;
    EXPECT(pv_koala_set_band_profile(h, lo.data(), hi.data()) == PV_STATUS_SUCCESS && drain() == 0);
    int16_t in[256], out[256];
    for (int i = 0; i < 256; ++i) in[i] = (int16_t) (i * 37);
    EXPECT(pv_koala_process(h, in, out) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_reset(h) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_get_band_profile(h, a.data(), b.data()) == PV_STATUS_SUCCESS && a == lo && b == hi);  // a reset is no change of configuration
    EXPECT(pv_koala_set_band_profile(h, nullptr, nullptr) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_get_band_profile(h, a.data(), nullptr) == PV_STATUS_SUCCESS && a[3] == 0.0f);
    pv_koala_delete(h);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <model.kns>\n", argv[0]);
        return 2;
    }
    batch(argv[1]);
    refusals(argv[1]);
    single_stream(argv[1]);
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}
