// A fractional handle's two stages around the REAL kernel source, the inner 16 kHz packet path replaced by a delay of 511 samples: three
// streams at different phases, per-call counts from {0, 1, 2, 3, 440, 441, 442, 882, max}, caller rows and inner rows with canaries behind
// every written extent, histories and phases in vectors of exactly their size (a touch outside is the sanitizer's to find), a masked reset
// mid-run.  Every output must equal a plain loop of the definition over the whole stream, and the phases the host mirror.
// usage: emu <U: 160 or 320>
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
static std::vector<double> prototype() {  // DESIGN.md section 2: the prototype of K = 441, in double
    const int K = 441, L = 48 * K + 1, c = 24 * K;
    const double pi = 3.141592653589793;
    std::vector<double> g(L);
    double sum = 0.0;
    for (int i = 0; i < L; ++i) {
        const double x = 0.94 * (i - c) / K, px = pi * x, sinc = i == c ? 1.0 : sin(px) / px;
        g[i] = sinc * (0.35875 - 0.48829 * cos(2.0 * pi * i / (L - 1)) + 0.14128 * cos(4.0 * pi * i / (L - 1)) - 0.01168 * cos(6.0 * pi * i / (L - 1)));
        sum += g[i];
    }
    for (double &v : g) v /= sum;
    return g;
}
static int16_t pcm(float a) { a = fminf(fmaxf(roundf(a), -32768.0f), 32767.0f); return (int16_t) (int) a; }
// the definition, over whole streams; a sample in front of the stream reads +0
static std::vector<int16_t> ref_in(const std::vector<int16_t> &x, const std::vector<float> &h, int U) {
    const long long M = x.empty() ? 0 : ((long long) U * (long long) x.size() - 1) / 441 + 1;
    std::vector<int16_t> y;
    for (long long m = 0; m < M; ++m) {
        float acc = 0.0f;
        for (long long i = 441 * m % U; i < (long long) h.size(); i += U) {
            const long long at = (441 * m - i) / U;
            acc = fmaf(h[i], at < 0 ? 0.0f : (float) x.at(at), acc);
        }
        y.push_back(pcm(acc));
    }
    return y;
}
static std::vector<int16_t> ref_out(const std::vector<int16_t> &v, size_t N, const std::vector<float> &h, int U, int c) {
    std::vector<int16_t> z;
    for (long long n = 0; n < (long long) N; ++n) {
        const long long p = (long long) U * n - c;
        float acc = 0.0f;
        for (long long i = ((p % 441) + 441) % 441; p >= 0 && i < (long long) h.size(); i += 441) {
            const long long at = (p - i) / 441;  // (p - i is a multiple of 441)
            acc = fmaf(h[i], at < 0 ? 0.0f : (float) v.at(at), acc);
        }
        z.push_back(pcm(acc));
    }
    return z;
}
int main(int argc, char **argv) {
    const int U = atoi(argv[1]), B = 3, Bpad = 16, maxs = 1000, T = fr_in_taps(U), C = fr_shift(U);
    if (U != 160 && U != 320) return 2;
    const int inner_max = (int) fr_inner(maxs, U);
    const std::vector<double> g = prototype();
    if ((int) g.size() != kFrTaps) return 2;
    std::vector<float> h_in(g.size()), h_out(g.size()), t_in((size_t) T * U, 0.0f), t_out((size_t) kFrOutTaps * 441, 0.0f);
    for (size_t i = 0; i < g.size(); ++i) h_in[i] = (float) (U * g[i]), h_out[i] = (float) (441 * g[i]);
    for (int j = 0; j < T; ++j) for (int r = 0; r < U && r + U * j < kFrTaps; ++r) t_in[(size_t) j * U + r] = h_in[r + U * j];
    for (int j = 0; j < kFrOutTaps; ++j) for (int r = 0; r < 441 && r + 441 * j < kFrTaps; ++r) t_out[(size_t) j * 441 + r] = h_out[r + 441 * j];
    std::vector<int16_t> hist_in((size_t) Bpad * T, 77), hist_out((size_t) Bpad * kFrOutHist, 77);
    std::vector<int32_t> ph_in(Bpad, 5), ph_out(Bpad, 5), counts(Bpad, 0), mirror(B, 0);
    std::vector<uint8_t> mask(Bpad, 0);
    FractionalStateArgs st{hist_in.data(), hist_out.data(), ph_in.data(), ph_out.data(), T, Bpad};
    launch((Bpad * (T + kFrOutHist) + 255) / 256, fractional_reset_kernel, st, (const uint8_t *) nullptr);
    for (int16_t v : hist_in) if (v) { printf("reset left history\n"); return 1; }
    std::vector<std::vector<int16_t>> x(B), y(B), v(B), z(B), delay(B, std::vector<int16_t>(kFrInnerDelay, 0));
    std::vector<int16_t> uin((size_t) B * maxs), uout((size_t) B * maxs), iin((size_t) B * inner_max), iout((size_t) B * inner_max);
    const int menu[] = {0, 1, 2, 3, 440, 441, 442, 882, maxs};
    srand(U);
    const int calls = 36;
    for (int call = 0; call < calls; ++call) {
        if (call == 20) {  // stream 1 restarts: what it has delivered so far is checked now, then it is a fresh stream
            mask[1] = 1;
            launch((Bpad * (T + kFrOutHist) + 255) / 256, fractional_reset_kernel, st, (const uint8_t *) mask.data());
            mask[1] = 0;
            if (z[1] != ref_out(v[1], x[1].size(), h_out, U, C) || y[1] != ref_in(x[1], h_in, U)) { printf("stream 1 before its reset\n"); return 1; }
            x[1].clear(), y[1].clear(), v[1].clear(), z[1].clear(), delay[1].assign(kFrInnerDelay, 0), mirror[1] = 0;
        }
        std::fill(uin.begin(), uin.end(), (int16_t) 11111);
        std::fill(iin.begin(), iin.end(), (int16_t) -7);
        std::fill(iout.begin(), iout.end(), (int16_t) 22222);
        std::fill(uout.begin(), uout.end(), (int16_t) -7);
        std::vector<int> m(B);
        for (int b = 0; b < B; ++b) {
            // the first calls put the streams out of phase: 1, 2 and 3 samples
            const int c = call == 0 ? b + 1 : call < 10 ? menu[(call + 3 * b) % 9] : menu[rand() % 9];
            counts[b] = c;
            m[b] = (int) (fr_inner(mirror[b] + c, U) - fr_inner(mirror[b], U));
            for (int i = 0; i < c; ++i) {
                const int16_t s = (int16_t) (rand() % 65536 - 32768);
                x[b].push_back(s), uin[(size_t) b * maxs + i] = s;
            }
        }
        const std::vector<int16_t> hin_before = hist_in, hout_before = hist_out;
        FractionalArgs a{uin.data(), iin.data(), counts.data(), hist_in.data(), ph_in.data(), t_in.data(), maxs, inner_max, U};
        if (U == 160) launch(B, fractional_in_kernel<160>, a); else launch(B, fractional_in_kernel<320>, a);
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i < inner_max; ++i) {
                const int16_t s = iin[(size_t) b * inner_max + i];
                if (i < m[b]) {  // the inner path: a delay of 511 samples
                    y[b].push_back(s);
                    delay[b].push_back(s);
                    iout[(size_t) b * inner_max + i] = delay[b].front();
                    v[b].push_back(delay[b].front());
                    delay[b].erase(delay[b].begin());
                } else if (s != -7) { printf("in-stage wrote past its count: call %d b %d i %d\n", call, b, i); return 1; }
            }
        }
        a = FractionalArgs{iout.data(), uout.data(), counts.data(), hist_out.data(), ph_out.data(), t_out.data(), inner_max, maxs, U};
        if (U == 160) launch(B, fractional_out_kernel<160>, a); else launch(B, fractional_out_kernel<320>, a);
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i < maxs; ++i) {
                const int16_t s = uout[(size_t) b * maxs + i];
                if (i < counts[b]) z[b].push_back(s);
                else if (s != -7) { printf("out-stage wrote past its count: call %d b %d i %d\n", call, b, i); return 1; }
            }
            mirror[b] = (mirror[b] + counts[b]) % 441;
            if (ph_in[b] != mirror[b] || ph_out[b] != mirror[b]) { printf("phase mismatch: call %d b %d\n", call, b); return 1; }
            if (counts[b] == 0 && (memcmp(&hist_in[(size_t) b * T], &hin_before[(size_t) b * T], T * 2) ||
                                   memcmp(&hist_out[(size_t) b * kFrOutHist], &hout_before[(size_t) b * kFrOutHist], kFrOutHist * 2))) {
                printf("a stalled stream's state moved: call %d b %d\n", call, b);
                return 1;
            }
        }
        for (int b = B; b < Bpad; ++b) if (ph_in[b] || ph_out[b]) { printf("padding stream touched\n"); return 1; }
    }
    for (int b = 0; b < B; ++b) {
        const std::vector<int16_t> wy = ref_in(x[b], h_in, U), wz = ref_out(v[b], x[b].size(), h_out, U, C);
        if (wy.size() != y[b].size()) { printf("stream %d: %zu inner samples, want %zu\n", b, y[b].size(), wy.size()); return 1; }
        for (size_t i = 0; i < wy.size(); ++i) if (wy[i] != y[b][i]) { printf("U %d stream %d inner sample %zu: got %d want %d\n", U, b, i, y[b][i], wy[i]); return 1; }
        for (size_t i = 0; i < wz.size(); ++i) if (wz[i] != z[b][i]) { printf("U %d stream %d output sample %zu: got %d want %d\n", U, b, i, z[b][i], wz[i]); return 1; }
        printf("stream %d: %zu inner and %zu output samples ok\n", b, wy.size(), wz.size());
    }
    return 0;
}
