// The peak limiter's member of the host-only engine double (tests/abi_sanitizer/engine_stub.cpp, which has every other one): g of a handle's
// streams lives in a table beside the double, 1 until it is set, so that what pv_limiter.cpp checks and forwards can be read back.
// TEST INFRASTRUCTURE: never linked into the product.
#include <map>

#include "kns_engine.h"

static std::map<const kns::Engine *, std::vector<float>> g_limiter_state;
int g_limiter_state_calls = 0;  // limiter_state calls that reached the engine

namespace kns {

Status Engine::limiter_state(bool set, int count, const int32_t *streams, float *state, std::string *err) {
    ++g_limiter_state_calls;
    if (getenv("STUB_FAIL_PROCESS")) {
        *err = "HIP error: stub";
        return Status::kRuntime;
    }
    for (int i = 0; streams && i < count; ++i)
        if (streams[i] < 0 || streams[i] >= B_) {
            *err = "`streams[" + std::to_string(i) + "]` = " + std::to_string(streams[i]) + " is outside [0, " + std::to_string(B_) + ").";
            return Status::kBadArgument;
        }
    std::vector<float> &all = g_limiter_state[this];
    if (all.empty()) all.assign((size_t) B_, 1.0f);
    for (int i = 0; i < count; ++i) {
        const int b = streams ? streams[i] : i;
        (set ? all[b] : state[i]) = set ? state[i] : all[b];
    }
    return Status::kOk;
}

}  // namespace kns
