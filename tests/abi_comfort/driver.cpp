// Drives comfort noise's entry points of the C ABI (include/pv_koala_batch.h: pv_koala_batch_set_comfort_noise / _get_comfort_noise,
// pv_koala_batch_get_comfort_state / _set_comfort_state, pv_koala_set_comfort_noise / _get_comfort_noise): validation entry by entry and
// bin by bin, NULL and out-of-range arguments, "a refused call changes nothing", the growth of struct_size, the four "not yet" refusals
// with an untouched output, and the getters.  Linked with koala_amd/csrc/pv_api*.cpp and the host-only engine double
// (tests/abi_sanitizer/engine_stub.cpp); the two translation units that list does not name -- koala_amd/csrc/pv_comfort.cpp, the code under
// test, and comfort noise's member of the double, engine_comfort_stub.cpp -- are included at the end of this file.  No GPU, no HIP
// runtime.  Exit status 0 = every expectation held.  usage: driver <model.kns>
#include <math.h>

#include <limits>

#include "../abi_sanitizer/expect.h"

extern int g_comfort_state_calls;

static const int K = PV_KOALA_NUM_BINS;

static pv_koala_comfort_t setting(int on, uint32_t seed) {
    pv_koala_comfort_t s;
    memset(&s, 0, sizeof(s));
    s.struct_size = (int32_t) sizeof(s), s.on = on, s.seed = seed;
    return s;
}

static void batch(const char *model) {
    const int B = 5, T = 2;
    pv_koala_batch_t *h = nullptr;
    EXPECT(pv_koala_batch_init("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, &h) == PV_STATUS_SUCCESS && h != nullptr);
    if (!h) return;
    std::string msg;
    std::vector<pv_koala_comfort_t> want(B, setting(0, 0)), tab;
    std::vector<float> want_amp((size_t) B * K, 0.0f), amp((size_t) B * K);
    for (int b = 0; b < B; ++b) tab.push_back(setting(1, 100u + b));
    for (size_t i = 0; i < amp.size(); ++i) amp[i] = 0.001f * (float) (i % 97);
    auto same = [&] {
        for (int b = 0; b < B; ++b) {
            pv_koala_comfort_t got = setting(7, 7);
            std::vector<float> a(K, -1.0f);
            if (pv_koala_batch_get_comfort_noise(h, b, &got, a.data()) != PV_STATUS_SUCCESS || drain() != 0) return false;
            if (got.on != want[b].on || got.seed != want[b].seed || memcmp(a.data(), &want_amp[(size_t) b * K], K * sizeof(float))) return false;
        }
        return true;
    };
    EXPECT(same());  // a new handle: every stream off, every curve zero

    // ---- refused: status, one message, nothing changed
    EXPECT(pv_koala_batch_set_comfort_noise(nullptr, B, nullptr, tab.data(), amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_set_comfort_noise(h, B, nullptr, nullptr, amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`settings`"));
    EXPECT(pv_koala_batch_get_comfort_noise(nullptr, 0, nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    for (int32_t bad : {-1, B, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()})
        EXPECT(pv_koala_batch_get_comfort_noise(h, bad, nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`stream`"));
    for (int32_t count : {0, -1, B + 1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()})
        EXPECT(pv_koala_batch_set_comfort_noise(h, count, nullptr, tab.data(), amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`count`"));
    std::vector<int32_t> idx(B);
    for (int32_t bad : {-1, B, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()}) {
        for (int i = 0; i < B; ++i) idx[i] = i;
        idx[3] = bad;
        EXPECT(pv_koala_batch_set_comfort_noise(h, B, idx.data(), tab.data(), amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`streams[3]`"));
        EXPECT(same());
    }
    for (int i = 0; i < B; ++i) idx[i] = i;
    idx[4] = 1;  // slot 1 twice; the entries in front of it are valid and must not have been applied
    EXPECT(pv_koala_batch_set_comfort_noise(h, B, idx.data(), tab.data(), amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "listed twice"));
    EXPECT(same());
    for (float v : {nanf(""), -1e-30f, -1.0f, INFINITY, -INFINITY}) {
        std::vector<float> bad(amp);
        bad[(size_t) 3 * K + 17] = v;
        EXPECT(pv_koala_batch_set_comfort_noise(h, B, nullptr, tab.data(), bad.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, "comfort 3, bin 17:"));
        EXPECT(same());
    }
    for (int32_t on : {2, -1}) {
        std::vector<pv_koala_comfort_t> bad(tab);
        bad[2].on = on;
        EXPECT(pv_koala_batch_set_comfort_noise(h, B, nullptr, bad.data(), amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "comfort 2:") &&
               has(msg, "`on`"));
        EXPECT(same());
    }
    for (int32_t size : {0, 8, 11, -12}) {
        std::vector<pv_koala_comfort_t> bad(tab);
        bad[0].struct_size = size;
        EXPECT(pv_koala_batch_set_comfort_noise(h, B, nullptr, bad.data(), amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`struct_size`"));
        EXPECT(same());
    }
    {
        std::vector<pv_koala_comfort_t> bad(tab);
        bad[1].struct_size = 16;
        EXPECT(pv_koala_batch_set_comfort_noise(h, B, nullptr, bad.data(), amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "comfort 1:"));
        EXPECT(same());
        pv_koala_comfort_t small = setting(0, 0);
        small.struct_size = 8;
        EXPECT(pv_koala_batch_get_comfort_noise(h, 0, &small, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`struct_size`"));
    }

    // ---- accepted: all streams; then a later header's wider entries for two slots, curves kept (amplitude == NULL); -0 is stored as +0
    EXPECT(pv_koala_batch_set_comfort_noise(h, B, nullptr, tab.data(), amp.data()) == PV_STATUS_SUCCESS && drain() == 0);
    want = tab, want_amp = amp;
    EXPECT(same());
    struct Wide {
        pv_koala_comfort_t s;
        int32_t later[2];
    } wide[2];
    memset(wide, 0x11, sizeof(wide));
    wide[0].s = setting(0, 5), wide[1].s = setting(1, 6);
    wide[0].s.struct_size = wide[1].s.struct_size = (int32_t) sizeof(Wide);
    const int32_t two[2] = {4, 0};
    EXPECT(pv_koala_batch_set_comfort_noise(h, 2, two, &wide[0].s, nullptr) == PV_STATUS_SUCCESS && drain() == 0);
    want[4] = setting(0, 5), want[0] = setting(1, 6);
    EXPECT(same());
    std::vector<float> row(K, 0.5f);
    row[9] = -0.0f;
    const int32_t slot = 2;
    pv_koala_comfort_t s2 = setting(1, 0xFFFFFFFFu);
    EXPECT(pv_koala_batch_set_comfort_noise(h, 1, &slot, &s2, row.data()) == PV_STATUS_SUCCESS);
    want[2] = s2;
    for (int k = 0; k < K; ++k) want_amp[(size_t) 2 * K + k] = k == 9 ? 0.0f : 0.5f;
    EXPECT(same());
    // the band profile a caller reads is still the neutral one
    std::vector<float> lo(K, -1.0f), hi(K, -1.0f);
    EXPECT(pv_koala_batch_get_band_profile(h, 1, lo.data(), hi.data()) == PV_STATUS_SUCCESS);
    for (int k = 0; k < K; ++k) EXPECT(lo[k] == 0.0f && hi[k] == 1.0f);

    // ---- the counters: checked lists, and values that come back
    std::vector<uint32_t> n(B, 9u);
    EXPECT(pv_koala_batch_get_comfort_state(nullptr, B, nullptr, n.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_get_comfort_state(h, B, nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`n`"));
    const int before = g_comfort_state_calls;
    for (int32_t count : {0, -1, B + 1}) EXPECT(pv_koala_batch_set_comfort_state(h, count, nullptr, n.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`count`"));
    EXPECT(g_comfort_state_calls == before);
    idx[4] = 1;
    EXPECT(pv_koala_batch_set_comfort_state(h, B, idx.data(), n.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "listed twice"));
    EXPECT(pv_koala_batch_get_comfort_state(h, B, nullptr, n.data()) == PV_STATUS_SUCCESS);
    for (uint32_t v : n) EXPECT(v == 0u);
    const uint32_t moved[2] = {0xFFFFFFFFu, 12u};
    EXPECT(pv_koala_batch_set_comfort_state(h, 2, two, moved) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_batch_get_comfort_state(h, B, nullptr, n.data()) == PV_STATUS_SUCCESS && n[4] == 0xFFFFFFFFu && n[0] == 12u && n[1] == 0u);

    // ---- calls, resets and records leave the configuration alone; the asynchronous entry points are refused while some stream is on
    std::vector<int16_t> in((size_t) B * T * 256, 3), out((size_t) B * T * 256, 0x5A5A);
    EXPECT(pv_koala_batch_process_chunk(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS && drain() == 0 && same());
    EXPECT(pv_koala_batch_reset(h, nullptr) == PV_STATUS_SUCCESS && same());
    int32_t bytes0 = 0, bytes1 = 0;
    EXPECT(pv_koala_batch_state_size(h, &bytes0) == PV_STATUS_SUCCESS && bytes0 > 0);
    std::fill(out.begin(), out.end(), (int16_t) 0x5A5A);
    EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "Comfort noise") &&
           has(msg, "asynchronous"));
    for (int16_t v : out) EXPECT(v == 0x5A5A);
    EXPECT(same());
    for (auto &s : tab) s.on = 0;
    EXPECT(pv_koala_batch_set_comfort_noise(h, B, nullptr, tab.data(), nullptr) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_batch_async_wait(h, 0) == PV_STATUS_SUCCESS);
    pv_koala_batch_t *plain = nullptr;
    EXPECT(pv_koala_batch_init("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, &plain) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_batch_state_size(plain, &bytes1) == PV_STATUS_SUCCESS && bytes1 == bytes0);
    pv_koala_batch_delete(plain);
    pv_koala_batch_delete(h);
}

// the other three "not yet" refusals: the channel link, the high-band carry, a handle at 44 100 Hz
static void refusals(const char *model) {
    std::string msg;
    pv_koala_comfort_t on = setting(1, 3);
    std::vector<float> amp(K, 0.01f);
    {
        pv_koala_batch_config_t cfg = config(4, 1, 0, 16000, PV_KOALA_SAMPLE_S16);
        pv_koala_batch_t *h = nullptr;
        EXPECT(pv_koala_batch_init_channels("k", model, "best", &cfg, 2, &h) == PV_STATUS_SUCCESS && h != nullptr);
        if (!h) return;
        std::vector<int16_t> in(4 * 256, 3), out(4 * 256, 0x5A5A);
        EXPECT(pv_koala_batch_set_channel_link(h, PV_KOALA_CHANNEL_LINK_MAX) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_set_comfort_noise(h, 1, nullptr, &on, amp.data()) == PV_STATUS_SUCCESS);  // setting it is configuration: accepted
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "Comfort noise") &&
               has(msg, "channel link"));
        for (int16_t v : out) EXPECT(v == 0x5A5A);
        EXPECT(pv_koala_batch_set_channel_link(h, PV_KOALA_CHANNEL_LINK_NONE) == PV_STATUS_SUCCESS);  // the link off: comfort noise alone
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_SUCCESS && drain() == 0);
        pv_koala_batch_delete(h);
    }
    {
        pv_koala_batch_t *h = nullptr;
        EXPECT(pv_koala_batch_init_rate("k", model, "best", 2, 1, PV_KOALA_PRECISION_FP32, 48000, &h) == PV_STATUS_SUCCESS && h != nullptr);
        if (!h) return;
        std::vector<int16_t> in(2 * 768, 3), out(2 * 768, 0x5A5A);
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_CARRY) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_set_comfort_noise(h, 1, nullptr, &on, amp.data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "Comfort noise") &&
               has(msg, "high-band carry"));
        for (int16_t v : out) EXPECT(v == 0x5A5A);
        EXPECT(pv_koala_batch_set_high_band(h, PV_KOALA_HIGH_BAND_NONE) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_chunk(h, 1, in.data(), out.data()) == PV_STATUS_SUCCESS && drain() == 0);
        pv_koala_batch_delete(h);
    }
    {
        pv_koala_batch_config_t cfg = config(2, 0, 441, 44100, PV_KOALA_SAMPLE_S16);
        pv_koala_batch_t *h = nullptr;
        EXPECT(pv_koala_batch_init_config("k", model, "best", &cfg, &h) == PV_STATUS_SUCCESS && h != nullptr);
        if (!h) return;
        std::vector<int16_t> in(2 * 441, 3), out(2 * 441, 0x5A5A);
        const int32_t counts[2] = {441, 441};
        pv_koala_batch_packets_t call;
        memset(&call, 0, sizeof(call));
        call.struct_size = (int32_t) sizeof(call), call.max_samples = 441, call.counts = counts, call.pcm = in.data(), call.enhanced = out.data();
        EXPECT(pv_koala_batch_set_comfort_noise(h, 1, nullptr, &on, amp.data()) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_packets(h, &call) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "Comfort noise") && has(msg, "44100"));
        for (int16_t v : out) EXPECT(v == 0x5A5A);
        on.on = 0;
        EXPECT(pv_koala_batch_set_comfort_noise(h, 1, nullptr, &on, nullptr) == PV_STATUS_SUCCESS);
        EXPECT(pv_koala_batch_process_packets(h, &call) == PV_STATUS_SUCCESS && drain() == 0);
        pv_koala_batch_delete(h);
    }
}

static void single_stream(const char *model) {
    pv_koala_t *h = nullptr;
    EXPECT(pv_koala_init("k", model, "best", &h) == PV_STATUS_SUCCESS && h != nullptr);
    if (!h) return;
    std::string msg;
    pv_koala_comfort_t s = setting(1, 42), got = setting(7, 7);
    std::vector<float> amp(K, 0.02f), back(K, -1.0f);
    EXPECT(pv_koala_get_comfort_noise(h, &got, back.data()) == PV_STATUS_SUCCESS && got.on == 0 && back[0] == 0.0f);
    EXPECT(pv_koala_set_comfort_noise(nullptr, &s, amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_get_comfort_noise(nullptr, &got, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_set_comfort_noise(h, nullptr, amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1);
    amp[256] = nanf("");
    EXPECT(pv_koala_set_comfort_noise(h, &s, amp.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "comfort 0, bin 256:"));
    EXPECT(pv_koala_get_comfort_noise(h, &got, nullptr) == PV_STATUS_SUCCESS && got.on == 0);
    amp[256] = 0.02f;
    EXPECT(pv_koala_set_comfort_noise(h, &s, amp.data()) == PV_STATUS_SUCCESS && drain() == 0);
    int16_t in[256], out[256];
    for (int i = 0; i < 256; ++i) in[i] = (int16_t) (i * 37);
    EXPECT(pv_koala_process(h, in, out) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_reset(h) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_get_comfort_noise(h, &got, back.data()) == PV_STATUS_SUCCESS && got.on == 1 && got.seed == 42u && back[256] == 0.02f);  // a reset is no change of configuration
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

// (see the head of the file)
#include "engine_comfort_stub.cpp"
#include "pv_comfort.cpp"
