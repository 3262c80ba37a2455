// The members of kns::Engine that koala_amd/csrc/pv_api_packets.cpp and pv_api_format.cpp call, for the sanitizer build of
// tests/abi_fractional_rate/driver.cpp: tests/abi_sanitizer/engine_stub.cpp is the host-only engine double and has none of them.  A packet
// handle "enables" by remembering its size, a fractional one its rate and size, a format its number; a call copies every stream's counted
// samples and counts itself.  TEST INFRASTRUCTURE: never linked into the product.
#include <string.h>

#include "kns_engine.h"

int g_packet_calls = 0;  // run_packets calls that reached the engine

namespace kns {

bool Engine::enable_packets(int max_samples, std::string *) {
    pk_max_ = max_samples;
    return true;
}

bool Engine::enable_fractional(int rate, int max_samples, std::string *) {
    fr_rate_ = rate, fr_max_ = max_samples;
    return true;
}

bool Engine::set_format(int fmt, std::string *) {
    fmt_ = fmt;
    return true;
}

Status Engine::run_packets(const PacketCall &c, std::string *) {
    ++g_packet_calls;
    const size_t eb = (size_t) sample_bytes();
    for (int b = 0; b < B_; ++b)
        memmove((uint8_t *) c.out + (size_t) b * c.max_samples * eb, (const uint8_t *) c.pcm + (size_t) b * c.max_samples * eb, (size_t) c.counts[b] * eb);
    return Status::kOk;
}

}  // namespace kns
