// Drives every entry point of the C ABI (include/pv_koala.h, include/picovoice.h, include/pv_koala_batch.h) through its argument
// checks, error-stack and ownership paths under AddressSanitizer + UndefinedBehaviorSanitizer, with the engine stubbed out
// (engine_stub.cpp).  The packet, format and 44.1 kHz entry points have drivers of their own (tests/abi_rational_rate,
// tests/abi_fractional_rate); their constructors' failure paths are here, with the channel entry points.  Exit status 0 = every expectation
// held and the sanitizers stayed silent, in this process and in the two it starts.  usage: driver <model.kns> <not-a-model>
#include <spawn.h>
#include <sys/wait.h>

#include <algorithm>
#include <thread>

#include "expect.h"

extern "C" {
void pv_set_sdk(const char *);
const char *pv_get_sdk(void);
void pv_free(void *);
void pv_log_enable(void);
void pv_log_disable(void);
extern char **environ;
}

static void single_stream(const char *model, const char *garbage) {
    pv_koala_t *h = nullptr;
    std::string msg;
    EXPECT(pv_koala_init(nullptr, model, "best", &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`access_key`") != std::string::npos);
    EXPECT(pv_koala_init("k", nullptr, "best", &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`model_path`") != std::string::npos);
    EXPECT(pv_koala_init("k", model, nullptr, &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`device`") != std::string::npos);
    EXPECT(pv_koala_init("k", model, "best", nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`object`") != std::string::npos);
    EXPECT(pv_koala_init("k", "/nonexistent/x.kns", "best", &h) == PV_STATUS_IO_ERROR && drain(&msg) == 2 && msg.find("Failed to open file") != std::string::npos);
    EXPECT(pv_koala_init("k", garbage, "best", &h) == PV_STATUS_IO_ERROR && drain() == 2);
    EXPECT(pv_koala_init("k", model, "foo", &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 2 && msg.find("foo is not a valid device string") != std::string::npos);
    EXPECT(pv_koala_init("k", model, "", &h) == PV_STATUS_INVALID_ARGUMENT && drain() == 2);
    EXPECT(pv_koala_init("k", model, "gpu:", &h) == PV_STATUS_INVALID_ARGUMENT && drain() == 2);
    EXPECT(pv_koala_init("k", model, "gpu:99999999999999999999", &h) == PV_STATUS_INVALID_ARGUMENT && drain() == 2);
    EXPECT(pv_koala_init("k", model, "cpu:4", &h) == PV_STATUS_RUNTIME_ERROR && drain() == 2);
    EXPECT(pv_koala_init("k", model, "gpu:7", &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 2 && msg.find("out of range") != std::string::npos);
    EXPECT(pv_koala_init("", model, "best", &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 2 && msg.find("AccessKey") != std::string::npos);
    // a very long device string must not overrun the message buffers
    std::string huge(5000, 'x');
    EXPECT(pv_koala_init("k", model, huge.c_str(), &h) == PV_STATUS_INVALID_ARGUMENT && drain() == 2);
    std::string huge_path = "/nonexistent/" + std::string(4000, 'p');
    EXPECT(pv_koala_init("k", huge_path.c_str(), "best", &h) == PV_STATUS_IO_ERROR && drain() == 2);
    setenv("STUB_GPUS", "0", 1);
    EXPECT(pv_koala_init("k", model, "best", &h) == PV_STATUS_RUNTIME_ERROR && drain() == 2);
    unsetenv("STUB_GPUS");
    setenv("STUB_OOM", "1", 1);
    EXPECT(pv_koala_init("k", model, "best", &h) == PV_STATUS_OUT_OF_MEMORY && drain() == 2);
    unsetenv("STUB_OOM");

    EXPECT(pv_koala_init("k", model, "gpu:0 - Stub GPU", &h) == PV_STATUS_SUCCESS && h != nullptr);
    EXPECT(drain() == 0);
    int16_t in[256], out[256];
    for (int i = 0; i < 256; ++i) in[i] = (int16_t) (i * 37);
    EXPECT(pv_koala_process(nullptr, in, out) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_process(h, nullptr, out) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_process(h, in, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_process(h, in, out) == PV_STATUS_SUCCESS && memcmp(in, out, sizeof(in)) == 0);
    EXPECT(pv_koala_process(h, in, in) == PV_STATUS_SUCCESS);  // in place
    setenv("STUB_FAIL_PROCESS", "1", 1);
    EXPECT(pv_koala_process(h, in, out) == PV_STATUS_RUNTIME_ERROR && drain() == 2);
    unsetenv("STUB_FAIL_PROCESS");
    setenv("STUB_THROW", "1", 1);  // an exception inside the engine must come back as a status, not cross the C ABI
    EXPECT(pv_koala_process(h, in, out) == PV_STATUS_OUT_OF_MEMORY && drain() == 1);
    unsetenv("STUB_THROW");
    // a failure's messages are replaced by the next call's (the stack describes the LAST call of the thread)
    EXPECT(pv_koala_process(nullptr, in, out) == PV_STATUS_INVALID_ARGUMENT);
    EXPECT(pv_koala_process(h, in, out) == PV_STATUS_SUCCESS && drain() == 0);
    int32_t delay = -1;
    EXPECT(pv_koala_delay_sample(nullptr, &delay) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_delay_sample(h, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_delay_sample(h, &delay) == PV_STATUS_SUCCESS && delay == 256);
    EXPECT(pv_koala_reset(nullptr) == PV_STATUS_INVALID_ARGUMENT);
    EXPECT(pv_koala_reset(h) == PV_STATUS_SUCCESS);
    pv_koala_delete(h);
    pv_koala_delete(nullptr);

    EXPECT(pv_koala_frame_length() == 256 && pv_sample_rate() == 16000 && !strcmp(pv_koala_version(), "3.0.0"));
    for (int s = -2; s < 16; ++s) EXPECT((pv_status_to_string((pv_status_t) s) != nullptr) == (s >= 0 && s <= 11));
    EXPECT(!strcmp(pv_status_to_string(PV_STATUS_SUCCESS), "SUCCESS"));
    EXPECT(pv_get_error_stack(nullptr, nullptr) != PV_STATUS_SUCCESS);
    pv_free_error_stack(nullptr);
    pv_free(nullptr);
    pv_free(malloc(8));
    EXPECT(!strcmp(pv_get_sdk(), "c"));
    pv_set_sdk("python");
    EXPECT(!strcmp(pv_get_sdk(), "python"));
    pv_set_sdk(nullptr);
    pv_set_sdk(std::string(3000, 's').c_str());
    EXPECT(strlen(pv_get_sdk()) > 0);
    pv_log_enable();
    pv_log_disable();

    char **devs = nullptr;
    int32_t ndev = -1;
    EXPECT(pv_koala_list_hardware_devices(nullptr, &ndev) == PV_STATUS_INVALID_ARGUMENT);
    EXPECT(pv_koala_list_hardware_devices(&devs, nullptr) == PV_STATUS_INVALID_ARGUMENT);
    (void) drain();
    EXPECT(pv_koala_list_hardware_devices(&devs, &ndev) == PV_STATUS_SUCCESS && ndev >= 1 && devs != nullptr);
    for (int i = 0; i < ndev; ++i) EXPECT(devs[i] != nullptr && strlen(devs[i]) > 0);
    pv_koala_free_hardware_devices(devs, ndev);
    pv_koala_free_hardware_devices(nullptr, 0);
}

static void batch(const char *model) {
    pv_koala_batch_t *b = nullptr;
    EXPECT(pv_koala_batch_init("k", model, "best", 0, 4, PV_KOALA_PRECISION_BF16, &b) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_init("k", model, "best", 3, 0, PV_KOALA_PRECISION_BF16, &b) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_init("k", model, "best", 3, 4, (pv_koala_precision_t) 7, &b) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_init("k", model, "best", 3, 4, PV_KOALA_PRECISION_BF16, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_init("k", model, "best", 3, 4, PV_KOALA_PRECISION_FP32, &b) == PV_STATUS_SUCCESS && b != nullptr);
    std::vector<int16_t> in(3 * 4 * 256, 5), out(3 * 4 * 256, 0);
    EXPECT(pv_koala_batch_process_chunk(nullptr, 4, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_process_chunk(b, 4, nullptr, out.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_process_chunk(b, 4, in.data(), nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_process_chunk(b, 0, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_process_chunk(b, 5, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_process_chunk(b, 4, in.data(), out.data()) == PV_STATUS_SUCCESS && out == in);
    EXPECT(pv_koala_batch_process(b, in.data(), out.data()) == PV_STATUS_SUCCESS);
    uint8_t mask[3] = {1, 0, 1};
    EXPECT(pv_koala_batch_reset(nullptr, mask) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_reset(b, mask) == PV_STATUS_SUCCESS && pv_koala_batch_reset(b, nullptr) == PV_STATUS_SUCCESS);
    int32_t n = 0, d = 0;
    EXPECT(pv_koala_batch_num_streams(b, &n) == PV_STATUS_SUCCESS && n == 3);
    EXPECT(pv_koala_batch_num_streams(b, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_num_streams(nullptr, &n) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_delay_sample(b, &d) == PV_STATUS_SUCCESS && d == 256);
    EXPECT(pv_koala_batch_delay_sample(nullptr, &d) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_set_stream(nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_set_stream(b, nullptr) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_batch_synchronize(nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_synchronize(b) == PV_STATUS_SUCCESS);
    double ms[5];
    int64_t launches[5];
    EXPECT(pv_koala_batch_profile_enable(nullptr, 1) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_profile_enable(b, 1) == PV_STATUS_SUCCESS);
    EXPECT(pv_koala_batch_profile_read(b, nullptr, launches) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_profile_read(b, ms, launches) == PV_STATUS_SUCCESS);
    float taps[4];
    EXPECT(pv_koala_batch_debug_read(nullptr, 0, taps, 4) < 0);
    EXPECT(pv_koala_batch_debug_read(b, 0, nullptr, 4) < 0);
    EXPECT(pv_koala_batch_debug_read(b, 99, taps, 4) < 0);
    void *pin = nullptr;
    EXPECT(pv_koala_batch_host_alloc(0, &pin) == PV_STATUS_INVALID_ARGUMENT && pin == nullptr && drain() == 1);
    EXPECT(pv_koala_batch_host_alloc(64, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_host_alloc(64, &pin) == PV_STATUS_SUCCESS && pin != nullptr);
    memset(pin, 0, 64);
    pv_koala_batch_host_free(pin);
    pv_koala_batch_host_free(nullptr);
    pv_koala_batch_delete(b);
    pv_koala_batch_delete(nullptr);
}

// the calls that carry a mask or stream records: per-frame resets (both forms), held streams, state size / export / import
static void batch_calls_with_arguments(const char *model) {
    const int B = 3, T = 4;
    pv_koala_batch_t *b = nullptr;
    EXPECT(pv_koala_batch_init("k", model, "best", B, T, PV_KOALA_PRECISION_BF16, &b) == PV_STATUS_SUCCESS && b != nullptr);
    std::vector<int16_t> in(B * T * 256, 7), out(B * T * 256, 0);
    std::vector<uint8_t> reset(B * T, 0), hold(B, 0);
    reset[1 * T + 2] = 1;  // stream 1 restarts before frame 2
    hold[2] = 1;
    std::string msg;
    typedef pv_status_t (*masked_call)(pv_koala_batch_t *, int32_t, const int16_t *, int16_t *, const uint8_t *);
    const masked_call calls[3] = {pv_koala_batch_process_chunk_resets, pv_koala_batch_process_chunk_resets_async, pv_koala_batch_process_chunk_hold};
    for (int i = 0; i < 3; ++i) {
        const masked_call call = calls[i];
        const uint8_t *mask = i < 2 ? reset.data() : hold.data();
        EXPECT(call(nullptr, T, in.data(), out.data(), mask) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`object`") != std::string::npos);
        EXPECT(call(b, T, nullptr, out.data(), mask) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`pcm`") != std::string::npos);
        EXPECT(call(b, T, in.data(), nullptr, mask) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`enhanced`") != std::string::npos);
        EXPECT(call(b, 0, in.data(), out.data(), mask) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`num_frames` 0") != std::string::npos);
        EXPECT(call(b, T + 1, in.data(), out.data(), mask) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
        std::fill(out.begin(), out.end(), 0);
        EXPECT(call(b, T, in.data(), out.data(), mask) == PV_STATUS_SUCCESS && out == in && drain() == 0);
        EXPECT(call(b, T, in.data(), out.data(), nullptr) == PV_STATUS_SUCCESS && drain() == 0);  // no mask: the plain call
        setenv("STUB_FAIL_PROCESS", "1", 1);
        EXPECT(call(b, T, in.data(), out.data(), mask) == PV_STATUS_RUNTIME_ERROR && drain(&msg) == 2 &&
               msg.find(i == 1 ? "0000033A" : "00000337") != std::string::npos);
        unsetenv("STUB_FAIL_PROCESS");
        setenv("STUB_THROW", "1", 1);
        EXPECT(call(b, T, in.data(), out.data(), mask) == PV_STATUS_OUT_OF_MEMORY && drain() == 1);
        unsetenv("STUB_THROW");
    }
    // a refused call leaves nothing behind for the next one (the mask travels with its call)
    EXPECT(pv_koala_batch_process_chunk_resets(b, T + 1, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_process_chunk(b, T, in.data(), out.data()) == PV_STATUS_SUCCESS && drain() == 0);

    int32_t size = -1;
    EXPECT(pv_koala_batch_state_size(nullptr, &size) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`object`") != std::string::npos);
    EXPECT(pv_koala_batch_state_size(b, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`num_bytes`") != std::string::npos);
    EXPECT(pv_koala_batch_state_size(b, &size) == PV_STATUS_SUCCESS && size > 0 && size % 16 == 0 && drain() == 0);
    std::vector<uint8_t> records((size_t) B * size, 0xAB);
    const int32_t two[2] = {2, 0}, outside[2] = {0, B};
    EXPECT(pv_koala_batch_export_state(nullptr, 2, two, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`object`") != std::string::npos);
    EXPECT(pv_koala_batch_export_state(b, 2, two, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`records`") != std::string::npos);
    EXPECT(pv_koala_batch_export_state(b, 0, two, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("`count` 0") != std::string::npos);
    EXPECT(pv_koala_batch_export_state(b, B + 1, nullptr, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_export_state(b, 2, outside, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && msg.find("00000066") != std::string::npos);
    EXPECT(pv_koala_batch_export_state(b, 2, two, records.data()) == PV_STATUS_SUCCESS && records[0] == 0 && records[2 * size - 1] == 0 &&
           records[2 * size] == 0xAB && drain() == 0);
    EXPECT(pv_koala_batch_export_state(b, B, nullptr, records.data()) == PV_STATUS_SUCCESS && records.back() == 0 && drain() == 0);
    EXPECT(pv_koala_batch_import_state(nullptr, 2, two, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_import_state(b, 2, two, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_import_state(b, 0, two, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_import_state(b, B + 1, nullptr, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_import_state(b, 2, outside, records.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    EXPECT(pv_koala_batch_import_state(b, 2, two, records.data()) == PV_STATUS_SUCCESS && drain() == 0);
    EXPECT(pv_koala_batch_import_state(b, B, nullptr, records.data()) == PV_STATUS_SUCCESS && drain() == 0);
    setenv("STUB_FAIL_PROCESS", "1", 1);
    EXPECT(pv_koala_batch_export_state(b, 2, two, records.data()) == PV_STATUS_RUNTIME_ERROR && drain(&msg) == 2 && msg.find("0000033C") != std::string::npos);
    EXPECT(pv_koala_batch_import_state(b, 2, two, records.data()) == PV_STATUS_RUNTIME_ERROR && drain(&msg) == 2 && msg.find("0000033C") != std::string::npos);
    unsetenv("STUB_FAIL_PROCESS");
    setenv("STUB_THROW", "1", 1);
    EXPECT(pv_koala_batch_export_state(b, 2, two, records.data()) == PV_STATUS_OUT_OF_MEMORY && drain() == 1);
    EXPECT(pv_koala_batch_import_state(b, 2, two, records.data()) == PV_STATUS_OUT_OF_MEMORY && drain() == 1);
    unsetenv("STUB_THROW");
    pv_koala_batch_delete(b);

    // a model with a five-frame front-end takes per-frame resets at frame 0 only: a later one is refused before the engine sees the call
    setenv("STUB_FRONT_TAPS", "5", 1);
    EXPECT(pv_koala_batch_init("k", model, "best", B, T, PV_KOALA_PRECISION_BF16, &b) == PV_STATUS_SUCCESS && b != nullptr);
    unsetenv("STUB_FRONT_TAPS");
    EXPECT(pv_koala_batch_process_chunk_resets(b, T, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
           msg.find("`reset[1][2]`") != std::string::npos);
    EXPECT(pv_koala_batch_process_chunk_resets_async(b, T, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    reset[1 * T + 2] = 0;
    reset[1 * T] = 1;  // frame 0: accepted
    EXPECT(pv_koala_batch_process_chunk_resets(b, T, in.data(), out.data(), reset.data()) == PV_STATUS_SUCCESS && drain() == 0);
    EXPECT(pv_koala_batch_state_size(b, &size) == PV_STATUS_SUCCESS && size % 16 == 0);
    pv_koala_batch_delete(b);
}

// pv_koala_batch_init_channels and pv_koala_batch_channels: every refusal with its message, and what a finished handle reports and refuses
static void channels(const char *model) {
    const int T = 2;
    std::string msg;
    pv_koala_batch_t *h = nullptr;
    pv_koala_batch_config_t c = config(4, T, 0, 16000, PV_KOALA_SAMPLE_S16);
    for (int32_t bad : {0, 9}) {
        EXPECT(pv_koala_batch_init_channels("k", model, "best", &c, bad, &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
               has(msg, ("`channels` " + std::to_string(bad) + " is outside [1, 8].").c_str()) && h == nullptr);
    }
    c.num_streams = 6;
    EXPECT(pv_koala_batch_init_channels("k", model, "best", &c, 4, &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
           has(msg, "`num_streams` 6 is not a multiple of `channels` 4") && h == nullptr);
    EXPECT(pv_koala_batch_init_channels("k", model, "best", nullptr, 2, &h) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 &&
           has(msg, "Argument `config` is NULL.") && h == nullptr);
    int32_t v = -1;
    EXPECT(pv_koala_batch_init_channels("k", model, "best", &c, 1, &h) == PV_STATUS_SUCCESS && h != nullptr && drain() == 0);
    EXPECT(pv_koala_batch_channels(h, &v) == PV_STATUS_SUCCESS && v == 1);
    pv_koala_batch_delete(h);

    c.num_streams = 4;
    h = nullptr;
    EXPECT(pv_koala_batch_init_channels("k", model, "best", &c, 2, &h) == PV_STATUS_SUCCESS && h != nullptr && drain() == 0);
    if (!h) return;
    EXPECT(pv_koala_batch_channels(h, &v) == PV_STATUS_SUCCESS && v == 2);
    EXPECT(pv_koala_batch_num_streams(h, &v) == PV_STATUS_SUCCESS && v == 4);
    EXPECT(pv_koala_batch_channels(nullptr, &v) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "Argument `object` is NULL."));
    EXPECT(pv_koala_batch_channels(h, nullptr) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, "Argument `channels` is NULL."));
    // the asynchronous entry points refuse the handle, with one message and nothing written
    std::vector<int16_t> in(4 * T * 256, 3), out(4 * T * 256, (int16_t) -7);
    std::vector<uint8_t> reset(4 * T, 0);
    pv_koala_batch_call_t call;
    memset(&call, 0, sizeof(call));
    call.struct_size = (int32_t) sizeof(call);
    call.num_frames = T, call.pcm = in.data(), call.enhanced = out.data(), call.asynchronous = 1;
    const char *refusal = "Asynchronous calls are not available on a handle whose `channels` is 2, not 1.";
    EXPECT(pv_koala_batch_process_chunk_async(h, T, in.data(), out.data()) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, refusal));
    EXPECT(pv_koala_batch_process_chunk_resets_async(h, T, in.data(), out.data(), reset.data()) == PV_STATUS_INVALID_ARGUMENT &&
           drain(&msg) == 1 && has(msg, refusal));
    EXPECT(pv_koala_batch_process_call(h, &call) == PV_STATUS_INVALID_ARGUMENT && drain(&msg) == 1 && has(msg, refusal));
    for (int16_t o : out) EXPECT(o == -7);
    EXPECT(pv_koala_batch_process_chunk(h, T, in.data(), out.data()) == PV_STATUS_SUCCESS && out == in && drain() == 0);
    pv_koala_batch_delete(h);
}

// A constructor whose enable step fails (the child process of enable_failures below: STUB_FAIL_ENABLE is set, to 1 or to throw): the
// handle it had finished is deleted and *object is NULL, whether the step returned false or threw -- a handle left behind is the leak
// report that fails this process at its exit.  (At 44 100 Hz the first step to fail is the inner packet handle's.)
static void enable_failure_cases(const char *model) {
    const bool throws = !strcmp(getenv("STUB_FAIL_ENABLE"), "throw");
    int sentinel = 0;
    std::string msg;
    const pv_koala_batch_config_t with_format = config(3, 2, 0, 16000, PV_KOALA_SAMPLE_ULAW), at_44100 = config(3, 0, 1000, 44100, PV_KOALA_SAMPLE_S16),
                                  planar = config(4, 2, 0, 16000, PV_KOALA_SAMPLE_S16);
    for (int which = 0; which < 4; ++which) {
        pv_koala_batch_t *h = (pv_koala_batch_t *) &sentinel;
        const pv_status_t st = which == 0 ? pv_koala_batch_init_packets("k", model, "best", 3, 480, PV_KOALA_PRECISION_FP32, 16000, &h) :
                               which == 1 ? pv_koala_batch_init_config("k", model, "best", &with_format, &h) :
                               which == 2 ? pv_koala_batch_init_config("k", model, "best", &at_44100, &h) :
                                            pv_koala_batch_init_channels("k", model, "best", &planar, 2, &h);
        EXPECT(st == PV_STATUS_OUT_OF_MEMORY && h == nullptr);
        EXPECT(drain(&msg) == 1 && has(msg, "00000065") && has(msg, throws ? "Failed to allocate memory." : "(stub)"));
    }
}

// the cases above in a fresh child process each way, so that a handle that leaks there is reported at that process's exit
static void enable_failures(const char *self, const char *model) {
    for (const char *mode : {"1", "throw"}) {
        setenv("STUB_FAIL_ENABLE", mode, 1);
        char *const child[] = {(char *) self, (char *) model, (char *) "enable-failures", nullptr};
        pid_t pid = -1;
        int status = -1;
        EXPECT(posix_spawn(&pid, self, nullptr, nullptr, child, environ) == 0 && waitpid(pid, &status, 0) == pid);
        EXPECT(WIFEXITED(status) && WEXITSTATUS(status) == 0);
        unsetenv("STUB_FAIL_ENABLE");
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[2], "enable-failures")) {
        enable_failure_cases(argv[1]);
        if (g_fail) fprintf(stderr, "%d expectation(s) failed with STUB_FAIL_ENABLE=%s\n", g_fail, getenv("STUB_FAIL_ENABLE"));
        return g_fail ? 1 : 0;
    }
    single_stream(argv[1], argv[2]);
    batch(argv[1]);
    batch_calls_with_arguments(argv[1]);
    channels(argv[1]);
    enable_failures(argv[0], argv[1]);
    // the error stack is per thread: failures on other threads leave this one's untouched, and eight threads hammering the
    // argument checks must not race (the stack is thread_local, the SDK string is behind a mutex)
    EXPECT(pv_koala_process(nullptr, nullptr, nullptr) == PV_STATUS_INVALID_ARGUMENT);
    std::vector<std::thread> pool;
    for (int t = 0; t < 8; ++t)
        pool.emplace_back([&, t] {
            for (int i = 0; i < 200; ++i) {
                pv_koala_t *h = nullptr;
                if (pv_koala_init("k", "/nonexistent", "best", &h) != PV_STATUS_IO_ERROR || drain() != 2) ++g_fail;
                pv_set_sdk(t & 1 ? "a" : "b");
                (void) pv_get_sdk();
            }
            if (drain() != 0) ++g_fail;
        });
    for (auto &th : pool) th.join();
    EXPECT(drain() == 1);  // this thread's message from before the pool is still here
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}
