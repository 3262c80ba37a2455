// A packet handle's call sequence around the REAL kernel source, the inner frame call replaced by a delay of one frame that checks what it is
// given: random counts (zeros and full rows included), caller rows at odd sample offsets, the engine's plan, held rows that must be zeros,
// nothing written past counts[b], fill_in == fill_out == the host mirror after every call, report rows gathered per stream, a record
// exported, scrambled and imported mid-run.  The streams' outputs must be their inputs delayed by 2 F - 1 samples.
using namespace kns;
template <class K, class... A> void launch(int blocks, K kernel, A... a) {
    for (int b = 0; b < blocks; ++b) {
        blockIdx.x = b;
        pthread_barrier_init(&bar, nullptr, 256);
        std::vector<std::thread> th;
        for (int t = 0; t < 256; ++t) th.emplace_back([=] { threadIdx.x = t; kernel(a...); });
        for (auto &t : th) t.join();
        pthread_barrier_destroy(&bar);
    }
}
int main(int argc, char **argv) {
    const int F = atoi(argv[1]), B = 5, Bpad = 16, Tmax = atoi(argv[2]), maxs = atoi(argv[3]), calls = 14;
    const int total = calls * maxs;
    std::vector<std::vector<int16_t>> x(B), got(B), prev(B, std::vector<int16_t>(F, 0)), e(B);
    srand(F + maxs);
    for (auto &v : x) for (int i = 0; i < total; ++i) v.push_back((int16_t) (rand() % 60000 - 30000));
    std::vector<int16_t> pin(Bpad * F, 77), pout(Bpad * F, 77), fin((size_t) B * (Tmax + 1) * F, 99), fout((size_t) B * (Tmax + 1) * F, 99);
    std::vector<int32_t> fi(Bpad, 5), fo(Bpad, 5), tab(Bpad + 2 + Tmax + 1), hostfill(B, 0), pos(B, 0);
    std::vector<float> subrep((size_t) B * (Tmax + 1) * 4), rep((size_t) B * (Tmax + 1) * 4);
    std::vector<int16_t> uin((size_t) B * maxs + 1), uout((size_t) B * maxs + 1);
    PacketStateArgs s{pin.data(), pout.data(), fi.data(), fo.data(), nullptr, nullptr, 0, Bpad, F, 0};
    launch((Bpad * F + 255) / 256, packet_reset_kernel, s, (const uint8_t *) nullptr);
    std::vector<int> framecount(B, 0);
    for (int call = 0; call < calls; ++call) {
        std::vector<int> k(B), cuts{0};
        const int odd = call & 1;  // odd calls: user rows start one sample in (2-byte aligned only)
        for (int b = 0; b < B; ++b) {
            int c = rand() % 4 == 0 ? 0 : rand() % (maxs + 1);
            if (call % 7 == 3) c = maxs;
            c = std::min(c, total - pos[b]);
            tab[b] = c;
            k[b] = (hostfill[b] + c) / F;
            memcpy(uin.data() + odd + (size_t) b * maxs, x[b].data() + pos[b], c * 2);
        }
        std::vector<int> ks(k); std::sort(ks.begin(), ks.end());
        for (int v : ks) { if (v <= cuts.back()) continue; while (v - cuts.back() > Tmax) cuts.push_back(cuts.back() + Tmax); cuts.push_back(v); }
        const int nsub = cuts.size() - 1;
        if (cuts.back() > Tmax) { printf("kmax %d > Tmax\n", cuts.back()); return 1; }
        tab[Bpad] = nsub;
        for (size_t i = 0; i < cuts.size(); ++i) tab[Bpad + 1 + i] = cuts[i];
        PacketArgs a{uin.data() + odd, uout.data() + odd, tab.data(), pin.data(), pout.data(), fi.data(), fo.data(), fin.data(), subrep.data(), rep.data(),
                     Tmax + 1, maxs, B, Bpad, F};
        launch(B, packet_in_kernel, a);
        for (int l = 0; l < nsub; ++l) {  // the inner call: a delay by one frame, held streams untouched; every row is read
            const int c0 = cuts[l], T = cuts[l + 1] - c0;
            for (int b = 0; b < B; ++b) {
                const int16_t *in = fin.data() + (size_t) B * F * c0 + (size_t) b * T * F;
                int16_t *out = fout.data() + (size_t) B * F * c0 + (size_t) b * T * F;
                const bool held = k[b] < cuts[l + 1];
                for (int i = 0; i < T * F; ++i) if (held && in[i] != 0) { printf("held row not zero\n"); return 1; }
                if (held) { for (int i = 0; i < T * F; ++i) out[i] = 12345; continue; }
                for (int t = 0; t < T; ++t) {
                    memcpy(out + t * F, prev[b].data(), F * 2);
                    memcpy(prev[b].data(), in + t * F, F * 2);
                    float *r = subrep.data() + (size_t) B * c0 * 4 + ((size_t) b * T + t) * 4;
                    r[0] = b, r[1] = framecount[b]++, r[2] = 1, r[3] = 0;
                }
            }
        }
        a.frames = fout.data();
        std::fill(uout.begin(), uout.end(), (int16_t) -7);
        std::fill(rep.begin(), rep.end(), -1.0f);
        launch(B, packet_out_kernel, a);
        for (int b = 0; b < B; ++b) {
            const int c = tab[b];
            for (int i = 0; i < maxs; ++i) {
                const int16_t v = uout[odd + (size_t) b * maxs + i];
                if (i < c) got[b].push_back(v);
                else if (v != -7) { printf("wrote past count: call %d b %d i %d\n", call, b, i); return 1; }
            }
            for (int f = 0; f < k[b]; ++f) {
                const float *r = rep.data() + ((size_t) b * (Tmax + 1) + f) * 4;
                if (r[0] != b || r[1] != framecount[b] - k[b] + f) { printf("report row wrong b %d f %d: %g %g\n", b, f, r[0], r[1]); return 1; }
            }
            hostfill[b] = hostfill[b] + c - k[b] * F;
            pos[b] += c;
            if (fi[b] != hostfill[b] || fo[b] != hostfill[b]) { printf("fill mismatch\n"); return 1; }
        }
        if (call == calls / 2) {  // export stream 2, scramble it, import it back
            const uint32_t rb = (4 + 2 * (F - 1) + 15) / 16 * 16;
            std::vector<uint8_t> recs(rb, 0xee);
            std::vector<int32_t> recof(Bpad, -1);
            recof[2] = 0;
            PacketStateArgs st{pin.data(), pout.data(), fi.data(), fo.data(), recof.data(), recs.data(), rb, Bpad, F, 0};
            launch(Bpad, packet_state_kernel, st);
            for (uint32_t i = 4 + 2 * (F - 1); i < rb; ++i) if (recs[i]) { printf("padding not zero\n"); return 1; }
            for (int i = 0; i < F; ++i) pin[2 * F + i] = 31000, pout[2 * F + i] = 31000;
            fi[2] = fo[2] = 9999;
            st.import = 1;
            launch(Bpad, packet_state_kernel, st);
        }
    }
    for (int b = 0; b < B; ++b) {
        for (size_t i = 0; i < got[b].size(); ++i) {
            const int16_t want = (int) i < 2 * F - 1 ? 0 : x[b][i - (2 * F - 1)];
            if (got[b][i] != want) { printf("F %d stream %d sample %zu: got %d want %d\n", F, b, i, got[b][i], want); return 1; }
        }
        printf("stream %d: %zu samples ok\n", b, got[b].size());
    }
    return 0;
}
