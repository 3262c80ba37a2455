// The packet members of kns::Engine for the sanitizer build of tests/abi_rational_rate/driver.cpp: tests/abi_sanitizer/engine_stub.cpp is
// the host-only engine double and has none, and koala_amd/csrc/pv_api_packets.cpp (pv_koala_batch_init_packets) calls these two.  A packet
// handle "enables" by remembering its size; a call copies every stream's counted samples.  TEST INFRASTRUCTURE: never linked into the product.
#include <string.h>

#include "kns_engine.h"

namespace kns {

bool Engine::enable_packets(int max_samples, std::string *) {
    pk_max_ = max_samples;
    return true;
}

Status Engine::run_packets(const PacketCall &c, std::string *) {
    for (int b = 0; b < B_; ++b)
        memmove((int16_t *) c.out + (size_t) b * c.max_samples, (const int16_t *) c.pcm + (size_t) b * c.max_samples, (size_t) c.counts[b] * 2);
    return Status::kOk;
}

}  // namespace kns
