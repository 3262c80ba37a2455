// The output leveller's member of the host-only engine double (tests/abi_sanitizer/engine_stub.cpp, which has every other one): the state
// of a handle's streams lives in a table beside the double, fresh until it is set, so that what pv_level.cpp checks and forwards can be
// read back.  TEST INFRASTRUCTURE: never linked into the product.
#include <map>

#include "kns_engine.h"

static std::map<const kns::Engine *, std::vector<float>> g_level_state;
int g_level_state_calls = 0;  // level_state calls that reached the engine

namespace kns {

Status Engine::level_state(bool set, int count, const int32_t *streams, float *state, std::string *err) {
    ++g_level_state_calls;
    if (getenv("STUB_FAIL_PROCESS")) {
        *err = "HIP error: stub";
        return Status::kRuntime;
    }
    for (int i = 0; streams && i < count; ++i)
        if (streams[i] < 0 || streams[i] >= B_) {
            *err = "`streams[" + std::to_string(i) + "]` = " + std::to_string(streams[i]) + " is outside [0, " + std::to_string(B_) + ").";
            return Status::kBadArgument;
        }
    std::vector<float> &all = g_level_state[this];
    if (all.empty())
        for (int b = 0; b < B_; ++b) all.push_back(0.0f), all.push_back(1.0f);
    for (int i = 0; i < count; ++i) {
        const int b = streams ? streams[i] : i;
        for (int k = 0; k < 2; ++k) (set ? all[2 * b + k] : state[2 * i + k]) = set ? state[2 * i + k] : all[2 * b + k];
    }
    return Status::kOk;
}

}  // namespace kns
