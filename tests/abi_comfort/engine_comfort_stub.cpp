// Comfort noise's member of the host-only engine double (tests/abi_sanitizer/engine_stub.cpp, which has every other one): the frame
// counters of a handle's streams live in a table beside the double, 0 until they are set, so that what pv_comfort.cpp checks and forwards
// can be read back.  TEST INFRASTRUCTURE: never linked into the product.
#include <map>

#include "kns_engine.h"

static std::map<const kns::Engine *, std::vector<uint32_t>> g_comfort_state;
int g_comfort_state_calls = 0;  // comfort_state calls that reached the engine

namespace kns {

Status Engine::comfort_state(bool set, int count, const int32_t *streams, uint32_t *n, std::string *err) {
    ++g_comfort_state_calls;
    std::vector<uint8_t> listed((size_t) B_, 0);
    for (int i = 0; i < count; ++i) {
        const int b = streams ? streams[i] : i;
        if (b < 0 || b >= B_ || listed[b]) {
            *err = b < 0 || b >= B_ ? "`streams[" + std::to_string(i) + "]` = " + std::to_string(b) + " is outside [0, " + std::to_string(B_) + ")."
                                    : "`streams[" + std::to_string(i) + "]`: slot " + std::to_string(b) + " is listed twice.";
            return Status::kBadArgument;
        }
        listed[b] = 1;
    }
    std::vector<uint32_t> &all = g_comfort_state[this];
    if (all.empty()) all.assign((size_t) B_, 0u);
    for (int i = 0; i < count; ++i) {
        const int b = streams ? streams[i] : i;
        (set ? all[b] : n[i]) = set ? n[i] : all[b];
    }
    return Status::kOk;
}

}  // namespace kns
