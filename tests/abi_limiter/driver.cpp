// Drives the peak limiter's entry points of the C ABI (include/pv_koala_batch.h: pv_koala_batch_set_limiter / _get_limiter,
// pv_koala_batch_get_limiter_state / _set_limiter_state, pv_koala_set_limiter / _get_limiter): validation field by field, NULL and
// out-of-range arguments, "a refused call changes nothing", the stride by struct_size (a short and a long struct), the state's round trip
// and the single-stream handle.  Linked with koala_amd/csrc/pv_api*.cpp and the host-only engine double (tests/abi_sanitizer/engine_stub.cpp)
// by tests/sanitized_build.py, build_abi_driver; the two translation units its list does not name -- koala_amd/csrc/pv_limiter.cpp, the code
// under test, and the limiter's member of the double, engine_limiter_stub.cpp -- are included at the end of this file.  No GPU, no HIP
// runtime.  Exit status 0 = every expectation held and the sanitizers stayed silent.  usage: driver <model.kns>
#include <math.h>
#include <stddef.h>

#include <limits>

#include "../abi_sanitizer/expect.h"

extern int g_limiter_state_calls;

static pv_koala_limiter_t good(int on = 1, float ceiling = 29205.0f, float release = 0.00125f) {
    pv_koala_limiter_t s;
    memset(&s, 0, sizeof(s));
    s.struct_size = (int32_t) sizeof(s), s.on = on, s.ceiling = ceiling, s.release = release;
    return s;
}

static bool equal(const pv_koala_limiter_t &a, const pv_koala_limiter_t &b) {
    return a.on == b.on && memcmp(&a.ceiling, &b.ceiling, 4) == 0 && memcmp(&a.release, &b.release, 4) == 0;
}

// a caller built against a later header: the known fields first, two more words behind them
struct Longer {
    pv_koala_limiter_t known;
    float later[2];
};

static void batch(const char *model) {
    const int B = 5, T = 2;
    pv_koala_batch_t *h = nullptr;
    EXPECT(pv_koala_batch_init("k", model, "best", B, T, PV_KOALA_PRECISION_FP32, &h) == PV_STATUS_SUCCESS && h != nullptr);
    if (!h) return;
    std::string msg;
    std::vector<pv_koala_limiter_t> want(B, good(0, 32767.0f, 1.0f)), tab;
    for (int b = 0; b < B; ++b) tab.push_back(good(1, 1000.0f + (float) b, 1.0f / (float) (256 << b)));
    auto same = [&] {
        for (int b = 0; b < B; ++b) {
            pv_koala_limiter_t got = good(7, 7.0f, 0.7f);
            if (pv_koala_batch_get_limiter(h, b, &got) != PV_STATUS_SUCCESS || drain() != 0 || !equal(got, want[b])) return false;
        }
        return true;
    };
    EXPECT(same());  // a new handle: every stream off

    // ---- refused: status, one message, nothing changed
    EXPECT(pv_koala_batch_set_limiter(nullptr, B, nullptr, tab.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_set_limiter(h, B, nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`settings`"));
    EXPECT(pv_koala_batch_get_limiter(nullptr, 0, &tab[0]) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_get_limiter(h, 0, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`setting`"));
    for (int32_t bad : {-1, B, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()}) {
        pv_koala_limiter_t got = good();
        EXPECT(pv_koala_batch_get_limiter(h, bad, &got) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`stream`"));
    }
    for (int32_t count : {0, -1, B + 1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()})
        EXPECT(pv_koala_batch_set_limiter(h, count, nullptr, tab.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`count`"));
    std::vector<int32_t> idx(B);
    for (int32_t bad : {-1, B, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()}) {
        for (int i = 0; i < B; ++i) idx[i] = i;
        idx[3] = bad;
        EXPECT(pv_koala_batch_set_limiter(h, B, idx.data(), tab.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`streams[3]`"));
        EXPECT(same());
    }
    for (int i = 0; i < B; ++i) idx[i] = i;
    idx[4] = 1;  // slot 1 twice; the entries in front of it are valid and must not have been applied
    EXPECT(pv_koala_batch_set_limiter(h, B, idx.data(), tab.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "listed twice"));
    EXPECT(same());
    for (float v : {nanf(""), 0.0f, 0.999f, -1000.0f, 32767.5f, 65536.0f, INFINITY, -INFINITY}) {
        std::vector<pv_koala_limiter_t> bad(tab);
        bad[3].ceiling = v;
        EXPECT(pv_koala_batch_set_limiter(h, B, nullptr, bad.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "setting 3: `ceiling`"));
        EXPECT(same());
    }
    for (float v : {nanf(""), 0.0f, -0.001f, 1.0001f, INFINITY, -INFINITY}) {
        std::vector<pv_koala_limiter_t> bad(tab);
        bad[2].release = v;
        EXPECT(pv_koala_batch_set_limiter(h, B, nullptr, bad.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "setting 2: `release`"));
        EXPECT(same());
    }
    for (int32_t on : {-1, 2, std::numeric_limits<int32_t>::max()}) {
        std::vector<pv_koala_limiter_t> bad(tab);
        bad[4].on = on;
        EXPECT(pv_koala_batch_set_limiter(h, B, nullptr, bad.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "setting 4: `on`"));
        EXPECT(same());
    }
    // ---- struct_size: a short struct, a size that is no whole number of words, entries that disagree -- and nothing behind the first
    // sizeof(int32_t) bytes of a refused short struct is read (the sanitizer watches the heap block)
    for (int32_t size : {0, 4, 12, (int32_t) sizeof(pv_koala_limiter_t) - 1, (int32_t) sizeof(pv_koala_limiter_t) + 2, -16}) {
        int32_t *shorter = (int32_t *) malloc(sizeof(int32_t));
        *shorter = size;
        EXPECT(pv_koala_batch_set_limiter(h, 1, nullptr, (const pv_koala_limiter_t *) shorter) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, "`struct_size`"));
        free(shorter);
        EXPECT(same());
    }
    {
        std::vector<pv_koala_limiter_t> bad(tab);
        bad[1].struct_size += 4;
        EXPECT(pv_koala_batch_set_limiter(h, B, nullptr, bad.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "setting 1: `struct_size`"));
        EXPECT(same());
        pv_koala_limiter_t got = good();
        got.struct_size = (int32_t) sizeof(got) - 4;
        EXPECT(pv_koala_batch_get_limiter(h, 0, &got) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`struct_size`"));
    }

    // ---- accepted: all streams; then a listed subset, the others keep theirs; a long struct is walked by its own stride
    EXPECT(pv_koala_batch_set_limiter(h, B, nullptr, tab.data()) == PV_STATUS_SUCCESS && drain() == 0);
    want = tab;
    EXPECT(same());
    {
        std::vector<Longer> longer(2);
        const int32_t listed[2] = {4, 0};
        for (int i = 0; i < 2; ++i) {
            longer[i].known = good(i, 2000.0f + (float) i, 0.5f);
            longer[i].known.struct_size = (int32_t) sizeof(Longer);
            longer[i].later[0] = longer[i].later[1] = nanf("");
            want[listed[i]] = longer[i].known;
        }
        EXPECT(pv_koala_batch_set_limiter(h, 2, listed, &longer[0].known) == PV_STATUS_SUCCESS && drain() == 0);
        EXPECT(same());
        Longer got;
        memset(&got, 0x5A, sizeof(got));
        got.known.struct_size = (int32_t) sizeof(Longer);
        const Longer before = got;
        EXPECT(pv_koala_batch_get_limiter(h, 4, &got.known) == PV_STATUS_SUCCESS && equal(got.known, want[4]));
        EXPECT(memcmp(got.later, before.later, sizeof(got.later)) == 0 && got.known.struct_size == (int32_t) sizeof(Longer));  // nothing behind the known fields
    }
    // the bounds themselves are accepted
    {
        const pv_koala_limiter_t lo = good(1, 1.0f, std::numeric_limits<float>::denorm_min()), hi = good(1, 32767.0f, 1.0f);
        const int32_t one[1] = {2};
        EXPECT(pv_koala_batch_set_limiter(h, 1, one, &lo) == PV_STATUS_SUCCESS);
        want[2] = lo;
        EXPECT(same());
        EXPECT(pv_koala_batch_set_limiter(h, 1, one, &hi) == PV_STATUS_SUCCESS);
        want[2] = hi;
        EXPECT(same());
    }

    // ---- the state: checked here, listed through to the engine, read back
    std::vector<float> st(B, -1.0f);
    const int before_calls = g_limiter_state_calls;
    EXPECT(pv_koala_batch_get_limiter_state(nullptr, B, nullptr, st.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_batch_get_limiter_state(h, B, nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`state`"));
    EXPECT(pv_koala_batch_set_limiter_state(h, B, nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`state`"));
    for (int32_t count : {0, -1, B + 1, std::numeric_limits<int32_t>::min()})
        EXPECT(pv_koala_batch_get_limiter_state(h, count, nullptr, st.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`count`"));
    for (float v : {nanf(""), 0.0f, -0.5f, 1.0001f, INFINITY}) {
        std::vector<float> bad(B, 0.5f);
        bad[3] = v;
        EXPECT(pv_koala_batch_set_limiter_state(h, B, nullptr, bad.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "state 3: `g`"));
    }
    EXPECT(g_limiter_state_calls == before_calls);  // none of them reached the engine
    EXPECT(pv_koala_batch_get_limiter_state(h, B, nullptr, st.data()) == PV_STATUS_SUCCESS && drain() == 0);
    for (int b = 0; b < B; ++b) EXPECT(st[b] == 1.0f);
    {
        const int32_t listed[2] = {4, 1};
        const float g[2] = {0.25f, 0.75f};
        EXPECT(pv_koala_batch_set_limiter_state(h, 2, listed, g) == PV_STATUS_SUCCESS && drain() == 0);
        EXPECT(pv_koala_batch_get_limiter_state(h, B, nullptr, st.data()) == PV_STATUS_SUCCESS);
        EXPECT(st[4] == 0.25f && st[1] == 0.75f && st[0] == 1.0f && st[2] == 1.0f && st[3] == 1.0f);
        const int32_t bad[2] = {4, B};
        EXPECT(pv_koala_batch_set_limiter_state(h, 2, bad, g) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`streams[1]`"));
        float two[2] = {-1.0f, -1.0f};
        EXPECT(pv_koala_batch_get_limiter_state(h, 2, listed, two) == PV_STATUS_SUCCESS && two[0] == 0.25f && two[1] == 0.75f);
    }
    setenv("STUB_FAIL_PROCESS", "1", 1);
    EXPECT(pv_koala_batch_get_limiter_state(h, B, nullptr, st.data()) == PV_STATUS_RUNTIME_ERROR && drain() == 2);
    unsetenv("STUB_FAIL_PROCESS");

    // ---- configuration: a call, a reset and a switch off and on leave the other fields where they are
    {
        std::vector<int16_t> x((size_t) B * T * 256, 100), y(x.size());
        EXPECT(pv_koala_batch_process_chunk(h, T, x.data(), y.data()) == PV_STATUS_SUCCESS && drain() == 0);
        EXPECT(pv_koala_batch_reset(h, nullptr) == PV_STATUS_SUCCESS);
        EXPECT(same());
        std::vector<pv_koala_limiter_t> off(want);
        for (auto &s : off) s.on = 0, s.struct_size = (int32_t) sizeof(s);  // (two of them were set through the longer struct)
        EXPECT(pv_koala_batch_set_limiter(h, B, nullptr, off.data()) == PV_STATUS_SUCCESS);
        want = off;
        EXPECT(same());
        EXPECT(pv_koala_batch_process_chunk(h, T, x.data(), y.data()) == PV_STATUS_SUCCESS && drain() == 0);
    }
    pv_koala_batch_delete(h);
}

static void single(const char *model) {
    pv_koala_t *k = nullptr;
    EXPECT(pv_koala_init("k", model, "best", &k) == PV_STATUS_SUCCESS && k != nullptr);
    if (!k) return;
    std::string msg;
    pv_koala_limiter_t got = good(7, 7.0f, 0.7f);
    EXPECT(pv_koala_get_limiter(k, &got) == PV_STATUS_SUCCESS && equal(got, good(0, 32767.0f, 1.0f)));
    EXPECT(pv_koala_set_limiter(nullptr, &got) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_get_limiter(nullptr, &got) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`object`"));
    EXPECT(pv_koala_set_limiter(k, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`settings`"));
    EXPECT(pv_koala_get_limiter(k, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`setting`"));
    pv_koala_limiter_t bad = good(1, 40000.0f);
    EXPECT(pv_koala_set_limiter(k, &bad) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "`ceiling`"));
    EXPECT(pv_koala_get_limiter(k, &got) == PV_STATUS_SUCCESS && equal(got, good(0, 32767.0f, 1.0f)));
    const pv_koala_limiter_t on = good(1, 23197.0f, 1.0f / 1024.0f);
    EXPECT(pv_koala_set_limiter(k, &on) == PV_STATUS_SUCCESS && drain() == 0);
    EXPECT(pv_koala_get_limiter(k, &got) == PV_STATUS_SUCCESS && equal(got, on));
    std::vector<int16_t> x(256, 100), y(256);
    EXPECT(pv_koala_process(k, x.data(), y.data()) == PV_STATUS_SUCCESS && drain() == 0);
    EXPECT(pv_koala_reset(k) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_get_limiter(k, &got) == PV_STATUS_SUCCESS && equal(got, on));  // configuration: a reset leaves it
    pv_koala_delete(k);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <model.kns>\n", argv[0]);
        return 2;
    }
    batch(argv[1]);
    single(argv[1]);
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}

// (see the head of the file)
#include "engine_limiter_stub.cpp"
#include "pv_limiter.cpp"
