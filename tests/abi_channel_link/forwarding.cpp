// Do the call structs reach the engine with the channel-link setting?  Linked with koala_amd/csrc/pv_api*.cpp and a RECORDING copy of the
// host-only engine double: tests/test_channel_link_abi.py writes it from tests/abi_sanitizer/engine_stub.cpp (left as it is), with one line
// added to Engine::process and Engine::run_packets each that keeps the call in the variables declared below.  Under AddressSanitizer +
// UndefinedBehaviorSanitizer like its sibling.  Exit status 0 = every expectation held.  usage: forwarding <model.kns>
#include "../abi_sanitizer/expect.h"
#include "kns_engine.h"

namespace kns {
extern Call g_seen_call;
extern PacketCall g_seen_packets;
extern int g_seen_calls, g_seen_packet_calls;
}  // namespace kns

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <model.kns>\n", argv[0]);
        return 2;
    }
    const int B = 4, C = 2, T = 2, N = 160;
    pv_koala_batch_t *h = nullptr;
    pv_koala_batch_config_t c = config(B, T, 0, 16000, PV_KOALA_SAMPLE_S16);
    EXPECT(pv_koala_batch_init_channels("k", argv[1], "best", &c, C, &h) == PV_STATUS_SUCCESS && h != nullptr);
    std::vector<int16_t> in((size_t) B * T * 256, 3), out(in.size());
    std::vector<uint8_t> hold(B, 0), reset((size_t) B * T, 0);
    std::vector<float> back(B, -1.0f), g(B, 0.0f);
    auto frame_call = [&](int which) {
        const int before = kns::g_seen_calls;
        pv_status_t st = PV_STATUS_RUNTIME_ERROR;
        if (which == 0) st = pv_koala_batch_process_chunk(h, T, in.data(), out.data());
        if (which == 1) st = pv_koala_batch_process_chunk_resets(h, T, in.data(), out.data(), reset.data());
        if (which == 2) st = pv_koala_batch_process_chunk_hold(h, T, in.data(), out.data(), hold.data());
        if (which == 3) {
            pv_koala_batch_call_t call;
            memset(&call, 0, sizeof(call));
            call.struct_size = (int32_t) sizeof(call);
            call.num_frames = T, call.pcm = in.data(), call.enhanced = out.data();
            st = pv_koala_batch_process_call(h, &call);
        }
        EXPECT(st == PV_STATUS_SUCCESS && kns::g_seen_calls == before + 1);
    };
    // link off, no limit: the plain call -- no table, no link
    for (int w = 0; w < 4; ++w) {
        frame_call(w);
        EXPECT(kns::g_seen_call.opt.channel_link == 0 && kns::g_seen_call.opt.min_gain == nullptr);
    }
    // link on, no limit: the setting, and the gain table (all zero) with it -- the linked kernels read it
    EXPECT(pv_koala_batch_set_channel_link(h, PV_KOALA_CHANNEL_LINK_MAX) == PV_STATUS_SUCCESS);
    for (int w = 0; w < 4; ++w) {
        frame_call(w);
        EXPECT(kns::g_seen_call.opt.channel_link == 1 && kns::g_seen_call.opt.min_gain != nullptr);
        for (int b = 0; kns::g_seen_call.opt.min_gain && b < B; ++b) EXPECT(kns::g_seen_call.opt.min_gain[b] == 0.0f);
    }
    // link on beside a limit: the handle's gains and their revision
    g[1] = 0.5f;
    EXPECT(pv_koala_batch_set_min_gain(h, B, nullptr, g.data()) == PV_STATUS_SUCCESS);
    const unsigned rev0 = kns::g_seen_call.opt.min_gain_rev;
    frame_call(0);
    EXPECT(kns::g_seen_call.opt.channel_link == 1 && kns::g_seen_call.opt.min_gain && kns::g_seen_call.opt.min_gain[1] == 0.5f && kns::g_seen_call.opt.min_gain_rev != rev0);
    // link off again, the limit stays: the table still travels, the link does not
    EXPECT(pv_koala_batch_set_channel_link(h, PV_KOALA_CHANNEL_LINK_NONE) == PV_STATUS_SUCCESS);
    frame_call(0);
    EXPECT(kns::g_seen_call.opt.channel_link == 0 && kns::g_seen_call.opt.min_gain && kns::g_seen_call.opt.min_gain[1] == 0.5f);
    // a refused change leaves what the next call carries
    EXPECT(pv_koala_batch_set_channel_link(h, 2) == PV_STATUS_INVALID_ARGUMENT && drain() == 1);
    frame_call(3);
    EXPECT(kns::g_seen_call.opt.channel_link == 0);
    pv_koala_batch_delete(h);

    // ---- a packet handle: PacketCall
    c = config(B, 0, N, 16000, PV_KOALA_SAMPLE_S16);
    EXPECT(pv_koala_batch_init_channels("k", argv[1], "best", &c, C, &h) == PV_STATUS_SUCCESS && h != nullptr);
    std::vector<int16_t> pin((size_t) B * N, 5), pout(pin.size());
    std::vector<int32_t> counts(B, N);
    pv_koala_batch_packets_t call;
    memset(&call, 0, sizeof(call));
    call.struct_size = (int32_t) sizeof(call);
    call.max_samples = N, call.counts = counts.data(), call.pcm = pin.data(), call.enhanced = pout.data();
    auto packet_call = [&] {
        const int before = kns::g_seen_packet_calls;
        EXPECT(pv_koala_batch_process_packets(h, &call) == PV_STATUS_SUCCESS && kns::g_seen_packet_calls == before + 1);
    };
    packet_call();
    EXPECT(kns::g_seen_packets.opt.channel_link == 0 && kns::g_seen_packets.opt.min_gain == nullptr);
    EXPECT(pv_koala_batch_set_channel_link(h, PV_KOALA_CHANNEL_LINK_MAX) == PV_STATUS_SUCCESS);
    packet_call();
    EXPECT(kns::g_seen_packets.opt.channel_link == 1 && kns::g_seen_packets.opt.min_gain != nullptr && kns::g_seen_packets.opt.min_gain[0] == 0.0f);
    EXPECT(pv_koala_batch_set_channel_link(h, PV_KOALA_CHANNEL_LINK_NONE) == PV_STATUS_SUCCESS);
    packet_call();
    EXPECT(kns::g_seen_packets.opt.channel_link == 0 && kns::g_seen_packets.opt.min_gain == nullptr);
    pv_koala_batch_delete(h);
    if (g_fail) fprintf(stderr, "%d expectation(s) failed\n", g_fail);
    return g_fail ? 1 : 0;
}
