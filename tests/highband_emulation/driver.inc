// The REAL kernel source of kns_resample.hip and kns_highband.hip, call by call, on arrays that are heap allocations of exactly their
// documented size (an index outside a row or a state is the sanitizer's to find).  Inputs come from a fixed generator; inputs, outputs and
// states go to the file named last on the command line as "name type count\n" + raw values, for tests/high_band_emulator.py to compare with
// the numpy recipes.
// usage: emu rs <U> <D> <q_frame> <file>   one stage "up U, down D": B = 3, calls of 1, 1, 3, 2, 16 frames
//        emu hb <R> <file>                 the in-stage (1, R) and the carry behind it: B = 4, calls of 1, 1, 1, 3, 2, 1, 4 frames
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
static FILE *sink;
template <class T> static void dump(const char *name, const char *type, const T *p, size_t n) {
    fprintf(sink, "%s %s %zu\n", name, type, n);
    if (n) fwrite(p, sizeof(T), n, sink);
}
static void dump_int(const char *name, int v) { dump(name, "i32", &v, 1); }
// an array of exactly n elements on the heap
template <class T> struct Exact {
    T *p;
    size_t n;
    Exact(size_t n_, T fill) : p(new T[n_]), n(n_) { std::fill(p, p + n, fill); }
    ~Exact() { delete[] p; }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};
static uint32_t lcg_state = 20240229u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }
static int16_t uniform(int peak) { return (int16_t) ((int) (lcg() % (uint32_t) (2 * peak + 1)) - peak); }
static int16_t full_range() { return (int16_t) ((int) (lcg() % 65536u) - 32768); }
// stream 0: the full int16 range; 1: noise of peak 20000; 2: the rails, alternating with a random phase flip now and then; 3: +-1
static int16_t input(int b, size_t i) {
    static int flip = 0;
    if (b == 0) return full_range();
    if (b == 1) return uniform(20000);
    if (b == 2) { if (lcg() % 97 == 0) flip ^= 1; return ((i & 1) ^ (size_t) flip) ? (int16_t) 32767 : (int16_t) -32768; }
    return uniform(1);
}
// DESIGN.md section 2: the prototype of K in double, times U, rounded once, zero-padded
static void table(int K, int U, float *taps) {
    const int L = 48 * K + 1, c = 24 * K;
    const double pi = 3.141592653589793;
    std::vector<double> g(L);
    double sum = 0.0;
    for (int i = 0; i < L; ++i) {
        const double x = 0.94 * (i - c) / K, px = pi * x, sinc = i == c ? 1.0 : sin(px) / px;
        g[i] = sinc * (0.35875 - 0.48829 * cos(2.0 * pi * i / (L - 1)) + 0.14128 * cos(4.0 * pi * i / (L - 1)) - 0.01168 * cos(6.0 * pi * i / (L - 1)));
        sum += g[i];
    }
    for (int i = 0; i < kRsMaxTaps; ++i) taps[i] = i < L ? (float) (U * (g[i] / sum)) : 0.0f;
}
static bool run_stage(const ResampleArgs &a) {
    const int blocks = a.B * ((a.T * a.q_frame + 255) / 256);
#define EMU_RS(UU, DD)                                                    \
    if (a.U == UU && a.D == DD) {                                         \
        if (a.resets) launch(blocks, resample_kernel<UU, DD, true>, a);   \
        else launch(blocks, resample_kernel<UU, DD, false>, a);           \
        return true;                                                      \
    }
    EMU_RS(2, 1) EMU_RS(3, 1) EMU_RS(1, 2) EMU_RS(1, 3) EMU_RS(2, 3) EMU_RS(3, 2) EMU_RS(4, 3) EMU_RS(3, 4)
#undef EMU_RS
    return false;
}
static int run_rs(int U, int D, int qf) {
    const int B = 3, K = U > D ? U : D, H = 48 * K / U;
    ResampleArgs a{};
    table(K, U, a.taps);
    dump("taps", "f32", a.taps, (size_t) 48 * K + 1);
    Exact<int16_t> s0((size_t) B * H, 77), s1((size_t) B * H, -77);
    int16_t *st[2] = {s0.p, s1.p};
    launch((B * H + 255) / 256, resample_reset_kernel, st[0], st[1], H, (const uint8_t *) nullptr, B);
    dump("state0", "i16", st[0], s0.n), dump("state1", "i16", st[1], s1.n);
    const int calls[] = {1, 1, 3, 2, 16};
    int cur = 0;
    for (int c = 0; c < 5; ++c) {
        const int T = calls[c], n_in = T * qf * D, n_out = T * qf * U;
        Exact<uint8_t> mask(B, 0);
        if (c == 3) {  // stream 1 restarts
            mask.p[1] = 1;
            launch((B * H + 255) / 256, resample_reset_kernel, st[0], st[1], H, (const uint8_t *) mask.p, B);
        }
        Exact<int16_t> in((size_t) B * n_in, 0), out((size_t) B * n_out, -7);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < n_in; ++i) in.p[(size_t) b * n_in + i] = input(b, i);
        Exact<uint8_t> flags((size_t) B * T, 0);
        if (c == 2) flags.p[2 * T + 0] = flags.p[2 * T + 2] = 1;                // 3 frames: stream 2, frame 0 and the last
        if (c == 4) flags.p[0] = flags.p[T + 5] = flags.p[T + 6] = flags.p[T + 15] = 1;  // 16 frames: stream 0 frame 0; stream 1 frames 5, 6, the last
        a.in = in.p, a.out = out.p, a.state = st[cur], a.state_next = st[cur ^ 1];
        a.resets = c == 2 || c == 4 ? flags.p : nullptr;
        a.B = B, a.T = T, a.U = U, a.D = D, a.q_frame = qf;
        if (!run_stage(a)) return 2;
        cur ^= 1;
        dump_int("T", T);
        dump("mask", "u8", mask.p, mask.n);
        dump("flags", "u8", flags.p, a.resets ? flags.n : 0);
        dump("in", "i16", in.p, in.n), dump("out", "i16", out.p, out.n);
        dump("state", "i16", st[cur], (size_t) B * H);
    }
    return 0;
}
static int run_hb(int R) {
    const int B = 4, XH = hb_x_hist(R), F = kFrame * R, Hin = 48 * R;
    ResampleArgs a{};
    table(R, 1, a.taps);
    HighBandArgs h{};
    table(R, R, h.taps);
    Exact<int16_t> i0((size_t) B * Hin, 77), i1((size_t) B * Hin, -77);
    Exact<int16_t> x0((size_t) B * XH, 77), x1((size_t) B * XH, -77), y0((size_t) B * kHbYHist, 77), y1((size_t) B * kHbYHist, -77);
    Exact<float> g0((size_t) B * 2, 77.0f), g1((size_t) B * 2, -77.0f);
    int16_t *si[2] = {i0.p, i1.p}, *xs[2] = {x0.p, x1.p}, *ys[2] = {y0.p, y1.p};
    float *ss[2] = {g0.p, g1.p};
    launch((B * Hin + 255) / 256, resample_reset_kernel, si[0], si[1], Hin, (const uint8_t *) nullptr, B);
    launch((B * XH + 255) / 256, hbk::high_band_reset_kernel, xs[0], xs[1], ys[0], ys[1], ss[0], ss[1], XH, (const uint8_t *) nullptr, B);
    for (int k = 0; k < 2; ++k) dump("xs0", "i16", xs[k], x0.n), dump("ys0", "i16", ys[k], y0.n), dump("ss0", "f32", ss[k], g0.n);
    const int calls[] = {1, 1, 1, 3, 2, 1, 4};
    const float tables[2][4] = {{0.0f, 0.25f, 1.0f, 0.5f}, {1.0f, 0.0f, 0.25f, 0.7f}};
    int cur = 0, hcur = 0;
    for (int c = 0; c < 7; ++c) {
        const int T = calls[c];
        Exact<uint8_t> mask(B, 0);
        if (c == 5) {  // streams 0 and 3 restart
            mask.p[0] = mask.p[3] = 1;
            launch((B * Hin + 255) / 256, resample_reset_kernel, si[0], si[1], Hin, (const uint8_t *) mask.p, B);
            launch((B * XH + 255) / 256, hbk::high_band_reset_kernel, xs[0], xs[1], ys[0], ys[1], ss[0], ss[1], XH, (const uint8_t *) mask.p, B);
        }
        Exact<int16_t> x((size_t) B * T * F, 0), y((size_t) B * T * kFrame, -7), out((size_t) B * T * F, 0);
        Exact<float> report((size_t) B * T * 4, -1.0f), gains(B, 0.0f);
        Exact<uint8_t> flags((size_t) B * T, 0);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < T * F; ++i) x.p[(size_t) b * T * F + i] = input(b, i), out.p[(size_t) b * T * F + i] = b == 0 ? full_range() : uniform(20000);
        for (int i = 0; i < B * T; ++i) report.p[(size_t) i * 4 + 2] = (float) (lcg() % 65536u) * (257.0f / 65535.0f);
        const bool with_gains = c >= 2, with_flags = c == 4;
        const int link = c >= 3 ? 2 : 0;
        if (with_gains) memcpy(gains.p, tables[c >= 5], sizeof(tables[0]));
        if (with_flags) flags.p[1 * T] = flags.p[2 * T] = 1;  // frame 0 of streams 1 and 2
        a.in = x.p, a.out = y.p, a.state = si[cur], a.state_next = si[cur ^ 1], a.resets = with_flags ? flags.p : nullptr;
        a.B = B, a.T = T, a.U = 1, a.D = R, a.q_frame = kFrame;
        if (!run_stage(a)) return 2;
        cur ^= 1;
        dump_int("T", T), dump_int("link", link);
        dump("mask", "u8", mask.p, mask.n);
        dump("flags", "u8", flags.p, with_flags ? flags.n : 0);
        dump("gains", "f32", gains.p, with_gains ? gains.n : 0);
        dump("x", "i16", x.p, x.n), dump("y", "i16", y.p, y.n), dump("E", "i16", out.p, out.n), dump("report", "f32", report.p, report.n);
        h.x = x.p, h.y = y.p, h.out = out.p, h.report = report.p, h.min_gain = with_gains ? gains.p : nullptr, h.resets = a.resets;
        h.xs = xs[hcur], h.ys = ys[hcur], h.ss = ss[hcur], h.xs_next = xs[hcur ^ 1], h.ys_next = ys[hcur ^ 1], h.ss_next = ss[hcur ^ 1];
        h.B = B, h.T = T, h.R = R, h.link = link;
        if (R == 2) launch(B * T, hbk::high_band_kernel<2>, h); else launch(B * T, hbk::high_band_kernel<3>, h);
        hcur ^= 1;
        dump("out", "i16", out.p, out.n);
        dump("xs", "i16", xs[hcur], x0.n), dump("ys", "i16", ys[hcur], y0.n), dump("ss", "f32", ss[hcur], g0.n);
    }
    return 0;
}
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::string what = argv[1];
    sink = fopen(argv[argc - 1], "wb");
    if (!sink) return 2;
    int rc = 2;
    if (what == "rs" && argc == 6) rc = run_rs(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    if (what == "hb" && argc == 4 && (atoi(argv[2]) == 2 || atoi(argv[2]) == 3)) rc = run_hb(atoi(argv[2]));
    fclose(sink);
    if (rc == 0) printf("done\n");
    return rc;
}
