// kns_engine.cpp -- parameter loading/packing, HBM workspace and the per-chunk kernel sequence of the KNS-v1 engine.
//
// Sequence for one call of B streams x T frames (fp32: 23 launches, independent of T):
//   analysis -> front-end GEMM -> 4 x { input GEMM A -> recurrent A -> input GEMM B -> recurrent B -> head GEMM } -> synthesis
// (bf16 configuration, one-frame front-end: 20 -- the front-end is folded into the stage-input GEMMs and the narrow heads of stages 0
// and 1 ride in their layer-B recurrent launches; several frames of few streams: T + 14 -- the layers as a wavefront over (stage,
// frame); the dispatch table stands in front of Engine::run_device)
// which is the batched form of what one pv_koala_process call does for one stream and one frame
// (reference include/pv_koala.h:65-80; stage structure per lib/common/koala_params.pv).
#include "kns_engine.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>

namespace kns {

// ------------------------------------------------------------------------------------------------ parameter file

namespace {

bool read_vec(FILE *f, std::vector<float> *v, size_t n) {
    v->resize(n);
    return fread(v->data(), sizeof(float), n, f) == n;
}

}  // namespace

LoadResult load_params(const char *path, Params *p, std::string *err) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        *err = std::string("Failed to open file `") + path + "`.";
        return kLoadIo;
    }
    char magic[8];
    uint32_t hdr[14];
    bool ok = fread(magic, 1, 8, f) == 8;
    if (ok && memcmp(magic, "koala", 5) == 0) {
        // the reference's own parameter file (lib/common/koala_params.pv, magic "koala3.0.0"): closed fixed-point format
        fclose(f);
        *err = std::string("`") + path + "` is a reference Koala `.pv` model: its fixed-point format is not documented and "
               "is not supported; pass a KNS1 (.kns) parameter file.";
        return kLoadFormat;
    }
    ok = ok && fread(hdr, 4, 14, f) == 14 && memcmp(magic, "KNS1\0\0\0\0", 8) == 0;
    ok = ok && hdr[0] == 1 && hdr[1] == kNfft && hdr[2] == kFrame && hdr[3] == kBins && hdr[4] == kHidden &&
         hdr[5] == kStages && hdr[9] == kBins && hdr[10] == kFrame;
    if (!ok) {
        fclose(f);
        *err = std::string("`") + path + "` is not a Koala (KNS1) model file.";
        return kLoadFormat;
    }
    // KNS-v1.1: a front-end over the last N feature frames (header word 11; 0 and 1 both mean one).  Checked as the unsigned
    // word it is: a value with the top bit set must not become a negative count that passes the test and sizes a vector.
    p->front_taps = hdr[11] > 1 && hdr[11] <= (uint32_t) kMaxFrontTaps ? (int) hdr[11] : 1;
    if (hdr[11] > (uint32_t) kMaxFrontTaps) {
        fclose(f);
        *err = std::string("`") + path + "` has a front-end over " + std::to_string(hdr[11]) + " feature frames (at most " +
               std::to_string(kMaxFrontTaps) + " are supported).";
        return kLoadFormat;
    }
    if (hdr[12] != 0) {  // the CPU oracle's fixed-point emulation (tools/pv_hypotheses.py): not an engine feature
        fclose(f);
        *err = std::string("`") + path + "` asks for re-quantised pre-activations (KNS1 header word 12), which only the CPU oracle emulates.";
        return kLoadFormat;
    }
    const size_t G3 = 3 * kHidden;
    ok = read_vec(f, &p->mean, kBins) && read_vec(f, &p->scale, kBins) &&
         read_vec(f, &p->w_in, (size_t) p->front_taps * kBins * kHidden) && read_vec(f, &p->b_in, kHidden);
    for (int s = 0; ok && s < kStages; ++s) {
        Params::Stage &st = p->st[s];
        p->head[s] = (int) hdr[6 + s];
        st.d_in = s ? p->head[s - 1] : 0;
        st.d_out = p->head[s];
        if (st.d_out <= 0 || st.d_out > kBins) {
            ok = false;
            break;
        }
        ok = read_vec(f, &st.w_ih_a, (size_t) (st.d_in + kHidden) * G3) && read_vec(f, &st.b_ih_a, G3) &&
             read_vec(f, &st.w_hh_a, (size_t) kHidden * G3) && read_vec(f, &st.b_hh_a, G3) &&
             read_vec(f, &st.w_ih_b, (size_t) kHidden * G3) && read_vec(f, &st.b_ih_b, G3) &&
             read_vec(f, &st.w_hh_b, (size_t) kHidden * G3) && read_vec(f, &st.b_hh_b, G3) &&
             read_vec(f, &st.w_head, (size_t) kHidden * st.d_out) && read_vec(f, &st.b_head, (size_t) st.d_out);
    }
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok) {
        *err = "Failed to read parameter from file.";
        return kLoadFormat;
    }
    return kLoadOk;
}

// ------------------------------------------------------------------------------------------------ weight packing

namespace {

struct Seg {
    int k0, klen;
};
struct Tile {
    int c0, valid;
};

uint16_t to_bf16(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t) (u >> 16);
}

std::vector<Tile> dense_tiles(int n, int multiple) {
    std::vector<Tile> t;
    for (int c = 0; c < n; c += 16) t.push_back({c, n - c < 16 ? n - c : 16});
    while (t.size() % (size_t) multiple) t.push_back({0, 0});
    return t;
}

std::vector<Tile> gru_tiles() {  // [unit tile][gate]: what one lane needs for a hidden unit sits in adjacent tiles
    std::vector<Tile> t;
    for (int u = 0; u < kUnitTiles; ++u)
        for (int g = 0; g < 3; ++g) {
            int left = kHidden - u * 16;
            t.push_back({g * kHidden + u * 16, left < 16 ? left : 16});
        }
    return t;
}

// B-packed image of W[k][n] (row-major, leading dimension ldw): [n-tile][k-block][lane][16 B]
std::vector<uint8_t> pack_b(const float *W, int ldw, const std::vector<Seg> &segs, const std::vector<Tile> &tiles,
                            int precision) {
    const PrecInfo pi = prec_info(precision);
    int nb = 0;
    for (const Seg &s : segs) nb += ceil_div(s.klen, pi.kb);
    std::vector<uint8_t> out(tiles.size() * (size_t) nb * 1024, 0);
    for (size_t nt = 0; nt < tiles.size(); ++nt) {
        int blk = 0;
        for (const Seg &s : segs) {
            for (int b = 0; b < ceil_div(s.klen, pi.kb); ++b, ++blk) {
                uint8_t *dst = out.data() + (nt * nb + blk) * 1024;
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < pi.epl; ++e) {
                        const int kk = precision == kBf16 ? (lane >> 4) * 8 + e : e * 4 + (lane >> 4);
                        const int k = b * pi.kb + kk, n = lane & 15;
                        float v = 0.0f;
                        if (k < s.klen && n < tiles[nt].valid) v = W[(size_t) (s.k0 + k) * ldw + tiles[nt].c0 + n];
                        if (precision == kBf16) {
                            uint16_t h = to_bf16(v);
                            memcpy(dst + (lane * 8 + e) * 2, &h, 2);
                        } else {
                            memcpy(dst + (lane * 4 + e) * 4, &v, 4);
                        }
                    }
            }
        }
    }
    return out;
}

// row[n] = fma(a[j], W[j][n], row[n]), j ascending: one row of the front-end fold (4 x 257 x 271 x 813 fused multiply-adds per handle).
// Two bodies of the same IEEE operations: the x86-64-v3 one (vfmadd, ~0.1 s per handle) is entered only on a CPU that reports
// FMA and AVX2; the portable one calls fmaf (correct on any host, seconds per handle).  Nothing else in this file is compiled
// with wider ISA flags, and -ffp-contract=off keeps every other a * b + c of the packing code two roundings.
#if defined(__x86_64__)
__attribute__((target("fma,avx2"))) void fold_row_v3(float *row, const float *a, const float *W, int J, int N) {
    for (int j = 0; j < J; ++j) {
        const float aj = a[j];
        const float *wr = W + (size_t) j * N;
        for (int n = 0; n < N; ++n) row[n] = __builtin_fmaf(aj, wr[n], row[n]);
    }
}
#endif
void fold_row_portable(float *row, const float *a, const float *W, int J, int N) {
    for (int j = 0; j < J; ++j) {
        const float aj = a[j];
        const float *wr = W + (size_t) j * N;
        for (int n = 0; n < N; ++n) row[n] = fmaf(aj, wr[n], row[n]);
    }
}
void fold_row(float *row, const float *a, const float *W, int J, int N) {
#if defined(__x86_64__)
    static const bool v3 = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
    if (v3) return fold_row_v3(row, a, W, J, N);
#endif
    fold_row_portable(row, a, W, J, N);
}

// true if rows k >= k_from of a B-packed image with nb k-blocks per n-tile are all zero.  The bf16 recurrent kernels publish hidden
// sequences whose k = 271, 272 hold the constant 1 (the bias rows' operand, kBiasK0), and the narrow heads write their few values
// into the features' padding columns: every OTHER consumer of those operands relies on its packed weights being zero there.
bool rows_zero_from(const std::vector<uint8_t> &img, int nb, int k_from, int precision) {
    const PrecInfo pi = prec_info(precision);
    const size_t ntiles = img.size() / ((size_t) nb * 1024);
    for (size_t nt = 0; nt < ntiles; ++nt)
        for (int blk = k_from / pi.kb; blk < nb; ++blk)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < pi.epl; ++e) {
                    const int kk = precision == kBf16 ? (lane >> 4) * 8 + e : e * 4 + (lane >> 4);
                    if (blk * pi.kb + kk < k_from) continue;
                    const uint8_t *v = img.data() + (nt * nb + blk) * 1024 + (size_t) (lane * pi.epl + e) * pi.esz;
                    for (int q = 0; q < pi.esz; ++q)
                        if (v[q]) return false;
                }
    return true;
}

std::vector<float> pack_bias(const float *b, const std::vector<Tile> &tiles) {
    std::vector<float> out(tiles.size() * 16, 0.0f);
    for (size_t nt = 0; nt < tiles.size(); ++nt)
        for (int n = 0; n < tiles[nt].valid; ++n) out[nt * 16 + n] = b[tiles[nt].c0 + n];
    return out;
}

}  // namespace

int visible_gpu_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void) hipGetLastError();
        return 0;
    }
    return n;
}

std::string gpu_name(int device) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        (void) hipGetLastError();
        return "unknown";
    }
    if (prop.name[0]) return prop.name;
    return std::string("AMD GPU ") + prop.gcnArchName;  // some ROCm installs leave the marketing name empty
}

// ------------------------------------------------------------------------------------------------ engine

struct Engine::WeightImage {
    int device = 0;
    std::vector<void *> allocs;
    float *window = nullptr, *twiddle = nullptr, *mean = nullptr, *scale = nullptr, *b_in = nullptr;
    void *w_in = nullptr;
    StageDev sd[kStages]{};
    int nby[kStages] = {0, 0, 0, 0};
    ~WeightImage() {
        (void) hipSetDevice(device);
        for (void *p : allocs) (void) hipFree(p);
    }
};

namespace {
// content key of a parameter set: 64-bit multiply-xor over every tensor (15 MB: ~2 ms), plus the dimensions
uint64_t params_key(const Params &p) {
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t) p.front_taps;
    auto mix = [&](const std::vector<float> &v) {
        const size_t n = v.size();
        h = (h ^ n) * 0xff51afd7ed558ccdull;
        const uint32_t *u = (const uint32_t *) v.data();
        size_t i = 0;
        for (; i + 1 < n; i += 2) {
            const uint64_t w = (uint64_t) u[i] | ((uint64_t) u[i + 1] << 32);
            h = (h ^ w) * 0x9e3779b97f4a7c15ull;
            h ^= h >> 29;
        }
        if (i < n) h = (h ^ u[i]) * 0x9e3779b97f4a7c15ull;
    };
    mix(p.mean), mix(p.scale), mix(p.w_in), mix(p.b_in);
    for (int s = 0; s < kStages; ++s) {
        const Params::Stage &st = p.st[s];
        h = (h ^ (uint64_t) (st.d_in * 1024 + st.d_out)) * 0xff51afd7ed558ccdull;
        mix(st.w_ih_a), mix(st.b_ih_a), mix(st.w_hh_a), mix(st.b_hh_a), mix(st.w_ih_b), mix(st.b_ih_b), mix(st.w_hh_b), mix(st.b_hh_b),
            mix(st.w_head), mix(st.b_head);
    }
    return h;
}
struct ImageKey {
    uint64_t content;
    int device, precision;
    bool operator<(const ImageKey &o) const {
        return content != o.content ? content < o.content : device != o.device ? device < o.device : precision < o.precision;
    }
};
std::mutex g_image_mutex;
std::map<ImageKey, std::weak_ptr<void>> g_images;  // (weak: an image lives as long as a handle holds it)

// every HIP failure the engine reports reads "HIP error: <the runtime's text>"
std::string hip_error(hipError_t e) { return std::string("HIP error: ") + hipGetErrorString(e); }
std::string hip_last_error() { return hip_error(hipGetLastError()); }
}  // namespace

// The prototype low-pass of the sample-rate stages (third extension), in double: g[0 ... 48 K].
static std::vector<double> rs_prototype_g(int K) {
    const int L = 2 * kRsHalf * K + 1, c = kRsHalf * K;
    const double pi = 3.141592653589793;
    std::vector<double> g0((size_t) L);
    double sum = 0.0;
    for (int i = 0; i < L; ++i) {
        const double x = 0.94 * (i - c) / K, px = pi * x;
        const double sinc = i == c ? 1.0 : sin(px) / px;
        const double w = 0.35875 - 0.48829 * cos(2.0 * pi * i / (L - 1)) + 0.14128 * cos(4.0 * pi * i / (L - 1)) -
                         0.01168 * cos(6.0 * pi * i / (L - 1));
        g0[i] = sinc * w;
        sum += g0[i];
    }
    for (int i = 0; i < L; ++i) g0[i] = g0[i] / sum;
    return g0;
}

// ... rounded once into the table h_U[i] = (float) (U g[i]) of a stage "up U, down D", zero-padded
static std::vector<float> rs_table(RsStage s) {
    const std::vector<double> g = rs_prototype_g(std::max(s.U, s.D));
    std::vector<float> h((size_t) kRsMaxTaps, 0.0f);
    for (size_t i = 0; i < g.size(); ++i) h[i] = (float) (s.U * g[i]);
    return h;
}

void *Engine::dalloc(size_t bytes, bool zero) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) {
        (void) hipGetLastError();
        alloc_failed_ = true;
        return nullptr;
    }
    (alloc_sink_ ? *alloc_sink_ : allocs_).push_back(p);
    // (on the handle's own non-blocking stream: a legacy-stream operation would collide with another handle's graph capture)
    if (zero) (void) hipMemsetAsync(p, 0, bytes, own_stream_);
    return p;
}

void *Engine::upload(const void *src, size_t bytes) {
    void *p = dalloc(bytes, false);
    if (p) {
        (void) hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, own_stream_);
        (void) hipStreamSynchronize(own_stream_);  // `src` is usually a temporary
    }
    return p;
}

Engine *Engine::create(const Params &p, int device, int num_streams, int max_frames, int precision, std::string *err,
                       bool *oom) {
    // (the handle is owned from its first byte: an exception out of init() -- std::bad_alloc from the packing vectors -- destroys the
    // stream, events and device allocations made so far and reaches the ABI as "out of memory", not as a leak)
    std::unique_ptr<Engine> e(new Engine());
    *oom = false;
    try {
        if (!e->init(p, device, num_streams, max_frames, precision, err, oom)) return nullptr;
    } catch (const std::bad_alloc &) {
        *oom = true;
        *err = "Failed to allocate host memory.";
        return nullptr;
    }
    return e.release();
}

// Tables and packed weights of one (model, device, precision): runs once per image, under g_image_mutex, with dalloc() recording into
// the image (alloc_sink_); leaves the pointers in this handle's members, from where init() copies them into the image.
bool Engine::build_weights(const Params &p, int precision, std::string *err) {
    // ---- tables
    std::vector<float> win(kNfft), tw(2 * kNfft);
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < kNfft; ++n) {
        win[n] = (float) sin(pi * (double) n / kNfft);
        tw[2 * n] = (float) cos(2.0 * pi * (double) n / kNfft);
        tw[2 * n + 1] = (float) -sin(2.0 * pi * (double) n / kNfft);
    }
    d_window_ = (float *) upload(win.data(), win.size() * 4);
    d_twiddle_ = (float *) upload(tw.data(), tw.size() * 4);
    d_mean_ = (float *) upload(p.mean.data(), kBins * 4);
    d_scale_ = (float *) upload(p.scale.data(), kBins * 4);

    // ---- weights, pre-packed into MFMA B-fragment order
    const int G3 = 3 * kHidden;
    if (!fold_) {
        auto tiles = dense_tiles(kHidden, pi_.npb);
        std::vector<Seg> segs;  // one segment per stacked feature frame, oldest first: each padded to whole k-blocks like the features
        for (int i = 0; i < p.front_taps; ++i) segs.push_back({i * kBins, kBins});
        auto w = pack_b(p.w_in.data(), kHidden, segs, tiles, precision);
        auto b = pack_bias(p.b_in.data(), tiles);
        w_in_ = upload(w.data(), w.size());
        b_in_ = (float *) upload(b.data(), b.size() * 4);
    }
    const auto gt = gru_tiles();
    bool pad_rows_ok = true;  // see rows_zero_from
    for (int s = 0; s < kStages; ++s) {
        const Params::Stage &st = p.st[s];
        StageDev &d = sd_[s];
        std::vector<Seg> segs_a;
        if (st.d_in) segs_a.push_back({0, st.d_in});
        segs_a.push_back({st.d_in, kHidden});
        // bf16 configuration: the gates are evaluated through 2^x, so the constants of
        // sigma(x) = 1 / (1 + 2^(-x log2 e)) and tanh(x) = 1 - 2 / (1 + 2^(2 x log2 e)) are folded into the r / z and n columns of
        // W_ih, W_hh and both biases BEFORE they are rounded to the operand type (one fp32 multiplication each; the oracle's
        // bf16 mode does the same): the recurrent kernels then add and exponentiate, nothing else
        auto gate_scaled = [&](const std::vector<float> &v, size_t rows) {
            std::vector<float> o(v);
            if (precision != kBf16) return o;
            for (size_t r = 0; r < rows; ++r)
                for (int c = 0; c < G3; ++c) o[r * G3 + c] = v[r * G3 + c] * (c < 2 * kHidden ? kGateScaleRZ : kGateScaleN);
            return o;
        };
        auto pk = [&](const std::vector<float> &w, const std::vector<Seg> &segs) {
            auto img = pack_b(gate_scaled(w, w.size() / G3).data(), G3, segs, gt, precision);
            // (the last segment is the hidden-sized one: its padding rows face the constant 1 of a published hidden sequence)
            int nb = 0;
            for (const Seg &sg : segs) nb += ceil_div(sg.klen, pi_.kb);
            pad_rows_ok = pad_rows_ok && rows_zero_from(img, nb, (nb - nbh_) * pi_.kb + kHidden, precision);
            return upload(img.data(), img.size());
        };
        auto pb = [&](const std::vector<float> &b) {
            auto img = pack_bias(gate_scaled(b, 1).data(), gt);
            return (float *) upload(img.data(), img.size() * 4);
        };
        // bf16 configuration: b_hh becomes rows kBiasK0, kBiasK0 + 1 of the packed W_hh -- the scaled bias as a bf16 pair, hi =
        // bf16(b), lo = bf16(b - hi) -- multiplied by the constant 1 every bf16 recurrent kernel keeps at those k of the hidden-state
        // operand (kns_layout.h; the oracle's bf16 mode appends the same two rows)
        auto pk_hh = [&](const std::vector<float> &w, const std::vector<float> &b) {
            if (precision != kBf16) return pk(w, {{0, kHidden}});
            std::vector<float> aug = gate_scaled(w, kHidden), bs = gate_scaled(b, 1);
            aug.resize((size_t) (kHidden + 2) * G3);
            for (int c = 0; c < G3; ++c) {
                const uint16_t hb = to_bf16(bs[c]);
                const uint32_t hu = (uint32_t) hb << 16;
                float hi;
                memcpy(&hi, &hu, 4);
                aug[(size_t) kBiasK0 * G3 + c] = hi;
                aug[(size_t) (kBiasK0 + 1) * G3 + c] = bs[c] - hi;  // (exact in fp32; rounded to bf16 by pack_b)
            }
            auto img = pack_b(aug.data(), G3, {{0, kHidden + 2}}, gt, precision);
            return upload(img.data(), img.size());
        };
        if (fold_) {
            // bf16 configuration, one-frame front-end: the front-end is linear and only the stage-input
            // GEMMs consume its output, so it is FOLDED into them -- with W_e the embedding rows of this stage's gate-scaled, unrounded
            // W_ih:  Wc[k][n] = sum_j w_in[k][j] W_e[j][n],  b'[n] = b_ih[n] + sum_j b_in[j] W_e[j][n]  (j ascending fmaf chains from 0, in
            // fp32), THEN rounded to bf16.  Stage input = [y_prev ; features]; the embedding is never formed.  (oracle: fold_front)
            const std::vector<float> ws = gate_scaled(st.w_ih_a, (size_t) st.d_in + kHidden), bs = gate_scaled(st.b_ih_a, 1);
            // a fed-forward head of at most kYPadMax values rides BEHIND the features and shares their last k-block (stages 1 and 2):
            // rows [features ; y_prev], ONE segment of 257 + d_in <= 288 rows; wider ones stay in front with k-blocks of their own
            d.ypad = st.d_in > 0 && st.d_in <= kYPadMax;
            const int f0 = d.ypad ? 0 : st.d_in, y0 = d.ypad ? kBins : 0;
            std::vector<float> wf((size_t) (st.d_in + kBins) * G3, 0.0f), bf(G3, 0.0f);
            memcpy(wf.data() + (size_t) y0 * G3, ws.data(), sizeof(float) * (size_t) st.d_in * G3);
            const float *we = ws.data() + (size_t) st.d_in * G3;
            for (int k = 0; k < kBins; ++k) fold_row(wf.data() + (size_t) (f0 + k) * G3, p.w_in.data() + (size_t) k * kHidden, we, kHidden, G3);
            for (int j = 0; j < kHidden; ++j)
                for (int n = 0; n < G3; ++n) bf[n] = __builtin_fmaf(p.b_in[j], we[(size_t) j * G3 + n], bf[n]);
            for (int n = 0; n < G3; ++n) bf[n] = bs[n] + bf[n];
            std::vector<Seg> segs_f;
            if (d.ypad) {
                segs_f.push_back({0, kBins + st.d_in});
            } else {
                if (st.d_in) segs_f.push_back({0, st.d_in});
                segs_f.push_back({st.d_in, kBins});
            }
            auto img = pack_b(wf.data(), G3, segs_f, gt, precision);
            {   // columns past [y ; features ; y behind] of the feature operand may hold other stages' head values
                int nb = 0;
                for (const Seg &sg : segs_f) nb += ceil_div(sg.klen, pi_.kb);
                pad_rows_ok = pad_rows_ok && rows_zero_from(img, nb, (nb - nbf_) * pi_.kb + kBins + (d.ypad ? st.d_in : 0), precision);
            }
            d.w_ih_a = upload(img.data(), img.size());
            auto bimg = pack_bias(bf.data(), gt);
            d.b_ih_a = (float *) upload(bimg.data(), bimg.size() * 4);
        } else {
            d.w_ih_a = pk(st.w_ih_a, segs_a);
            d.b_ih_a = pb(st.b_ih_a);
        }
        d.w_hh_a = pk_hh(st.w_hh_a, st.b_hh_a);
        d.w_ih_b = pk(st.w_ih_b, {{0, kHidden}});
        d.w_hh_b = pk_hh(st.w_hh_b, st.b_hh_b);
        d.b_hh_a = pb(st.b_hh_a);
        d.b_ih_b = pb(st.b_ih_b);
        d.b_hh_b = pb(st.b_hh_b);
        auto ht = dense_tiles(st.d_out, s < kStages - 1 ? pi_.npb : 1);
        auto hw = pack_b(st.w_head.data(), st.d_out, {{0, kHidden}}, ht, precision);
        pad_rows_ok = pad_rows_ok && rows_zero_from(hw, nbh_, kHidden, precision);
        auto hb = pack_bias(st.b_head.data(), ht);
        d.w_head = upload(hw.data(), hw.size());
        d.b_head = (float *) upload(hb.data(), hb.size() * 4);
        d.head_tiles = (int) ht.size();
        d.head_dim = st.d_out;
        nby_[s] = ceil_div(st.d_out, pi_.kb);
    }

    if (!pad_rows_ok) {
        *err = "Internal error: a packed weight image has non-zero padding rows.";
        return false;
    }
    return true;

}

bool Engine::init(const Params &p, int device, int B, int Tmax, int precision, std::string *err, bool *oom) {
    if (hipSetDevice(device) != hipSuccess) {
        (void) hipGetLastError();
        *err = "Failed to communicate with device.";
        return false;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        (void) hipGetLastError();
        *err = "Failed to communicate with device.";
        return false;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        *err = std::string("GPU `") + prop.gcnArchName + "` is not supported: this build carries gfx950 (MI355X) code only.";
        return false;
    }
    device_ = device;
    B_ = B;
    Bpad_ = ceil_div(B, 16) * 16;
    Tmax_ = Tmax;
    prec_ = precision;
    pi_ = prec_info(precision);
    nbf_ = ceil_div(kBins, pi_.kb);
    nbh_ = ceil_div(kHidden, pi_.kb);
    taps_ = p.front_taps;
    if (!rs_rate_ok(p.sample_rate)) {
        *err = "sample rate " + std::to_string(p.sample_rate) + " is not one of 8000, 12000, 16000, 24000, 32000, 48000.";
        return false;
    }
    rate_ = p.sample_rate;
    fold_ = precision == kBf16 && taps_ == 1;  // the front-end rides in the stage-input GEMMs (see the packing below)
    if (hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking) != hipSuccess) {
        (void) hipGetLastError();
        *err = "Failed to create a HIP stream.";
        return false;
    }
    stream_ = own_stream_;
    // developer switches: read once per handle, and only in the -DKNS_DEV build (dev_env() is a constant nullptr otherwise)
    use_graph_ = dev_env("KOALA_AMD_NO_GRAPH") == nullptr;
    no_small_ = dev_env("KOALA_AMD_NO_SMALL") != nullptr;
    no_zero_copy_ = dev_env("KOALA_AMD_NO_ZERO_COPY") != nullptr;
    no_recompute_ = dev_env("KOALA_AMD_STORE_SPECTRUM") != nullptr;  // A/B switch: spectrum through HBM in every call
    debug_taps_ = dev_env("KOALA_AMD_DEBUG_TAPS") != nullptr;        // keep every intermediate debug_read() can return
    dev_variant_ = (dev_env("KOALA_AMD_GRU_STREAM") ? kDevGruStream : 0) | (dev_env("KOALA_AMD_GEMM_GENERIC") ? kDevGemmGeneric : 0) |
                   (dev_env("KOALA_AMD_GEMM_NO_WSR") ? kDevGemmNoWsr : 0);
    auto dev_int = [](const char *name, int dflt) {
        const char *e = dev_env(name);
        return e ? atoi(e) : dflt;
    };
    dev_only_class_ = dev_int("KOALA_AMD_ONLY_CLASS", -1);  // power / clock probing: launch one kernel class only (garbage out)
    dev_analysis_seg_ = dev_int("KOALA_AMD_ANALYSIS_SEG", 0);
    dev_synth_seg_ = dev_int("KOALA_AMD_SYNTH_SEG", 0);
    dev_small_mt_ = dev_int("KOALA_AMD_SMALL_MT", 0);
    dev_steps_mt_ = dev_int("KOALA_AMD_STEPS_MT", 192);
    dev_wave_mt_ = dev_int("KOALA_AMD_WAVE_MT", -1);  // -1: the measured limits; 0: never
    dev_wave_group_ = dev_int("KOALA_AMD_WAVE_GROUP", 0);
    dev_wave_parts_ = dev_int("KOALA_AMD_WAVE_PARTS", 1);  // 0: a layer never takes more than one XCD
    dev_pipe_chunk_ = dev_int("KOALA_AMD_PIPE_CHUNK", 0);  // frames per sub-chunk of the layer pipeline of mid-size batches (0: 16)
    dev_pipe_whole_stft_ = dev_env("KOALA_AMD_PIPE_WHOLE_STFT") != nullptr;  // its analysis / synthesis as whole-call launches (A/B arm)
    dev_pipe_streams_ = dev_int("KOALA_AMD_PIPE_STREAMS", 0);  // streams of the pipeline (0: the default, at most 4)
    dev_pipe_grid_ = dev_int("KOALA_AMD_PIPE_GRID", 0);    // workgroups of its weight-stationary GEMM launches (0: the default)
    dev_pipe_mt_ = dev_int("KOALA_AMD_PIPE_MT", -1);       // up to this many m-tiles (-1: the measured limit; 0: never)
    // One-frame calls of large batches: a GRU layer as ONE launch fused over CU quads (kns_gruq.hip, gru_quad1_kernel), bit-identical
    // to the two-kernel form -- a CU pulls a quarter of W_ih and W_hh (300 KiB) per layer instead of a half of one and all of the
    // other (~740 KiB): 128 against 222 us per 4096-stream frame step.  (The multi-frame form of that decomposition measured slower
    // than input GEMM + recurrent kernel, 354 against 278 us per layer at 64 frames, and is no longer in the tree: DESIGN.md section 6.)
    use_quad_ = dev_env("KOALA_AMD_NO_QUAD") == nullptr;
    fuse_head_ = dev_env("KOALA_AMD_NO_HEAD_FUSE") == nullptr;
    fuse_front_ = dev_env("KOALA_AMD_NO_STFT_FUSE") == nullptr;  // A/B arm: front-end / mask head as launches of their own in one-frame calls  // A/B arm: narrow heads as launches of their own in one-frame calls
    quad_nb0_max_ = dev_int("KOALA_AMD_QUAD_NB0MAX", 2);
    qdbg_block_ = dev_int("KOALA_AMD_QUAD_DBG", -1);
    // host-pointer calls are cut into sub-chunks of host_chunk_ frames (two staging slots = the Tmax-sized buffers)
    host_chunk_ = Tmax_ / 2 < 1 ? 1 : (Tmax_ / 2 > 16 ? 16 : Tmax_ / 2);
    host_pipeline_min_bytes_ = (size_t) 4 << 20;  // below this a call is launch-bound: sub-chunks would only add launches
    if (const char *e = dev_env("KOALA_AMD_HOST_SCHED")) {  // sub-chunk lengths "6,8,12,...": repeated / truncated to the call's frames
        for (const char *q = e; *q;) {
            dev_host_sched_.push_back(atoi(q));
            while (*q && *q != ',') ++q;
            if (*q == ',') ++q;
        }
    }
    if (const char *e = dev_env("KOALA_AMD_HOST_CHUNK")) {  // force a sub-chunk length; 0 = never split
        const int v = atoi(e);
        if (v >= 1 && v <= Tmax_ / 2) host_chunk_ = v, host_pipeline_min_bytes_ = 0;
        if (v == 0) host_chunk_ = Tmax_;
    }
    bool ok_sync = hipStreamCreateWithFlags(&copy_in_, hipStreamNonBlocking) == hipSuccess &&
                   hipStreamCreateWithFlags(&copy_out_, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 2 && ok_sync; ++i)
        ok_sync = hipEventCreateWithFlags(&ev_in_[i], hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&ev_done_[i], hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&ev_out_[i], hipEventDisableTiming) == hipSuccess;
    if (!ok_sync) {
        (void) hipGetLastError();
        *err = "Failed to create HIP streams/events.";
        return false;
    }

    // ---- tables and weights: shared with every other handle open on the same model, device and precision
    {
        std::lock_guard<std::mutex> lock(g_image_mutex);
        model_key_ = params_key(p);
        const ImageKey key{model_key_, device, precision};
        std::shared_ptr<void> held = g_images[key].lock();
        // (KOALA_AMD_NO_WEIGHT_CACHE, developer build: every handle builds its own image, as in rounds 1-5)
        if (held && !dev_env("KOALA_AMD_NO_WEIGHT_CACHE")) {
            weights_ = std::static_pointer_cast<WeightImage>(held);
        } else {
            weights_ = std::make_shared<WeightImage>();
            weights_->device = device;
            alloc_sink_ = &weights_->allocs;
            const bool built = build_weights(p, precision, err);
            alloc_sink_ = nullptr;
            if (!built) return false;
            if (alloc_failed_) {
                *oom = true;
                *err = "Failed to allocate device memory.";
                return false;
            }
            WeightImage &w = *weights_;
            w.window = d_window_, w.twiddle = d_twiddle_, w.mean = d_mean_, w.scale = d_scale_, w.w_in = w_in_, w.b_in = b_in_;
            for (int s = 0; s < kStages; ++s) w.sd[s] = sd_[s], w.nby[s] = nby_[s];
            for (auto it = g_images.begin(); it != g_images.end();)  // (entries whose last handle is gone)
                it = it->second.expired() ? g_images.erase(it) : std::next(it);
            g_images[key] = std::static_pointer_cast<void>(weights_);
        }
        const WeightImage &w = *weights_;
        d_window_ = w.window, d_twiddle_ = w.twiddle, d_mean_ = w.mean, d_scale_ = w.scale, w_in_ = w.w_in, b_in_ = w.b_in;
        for (int s = 0; s < kStages; ++s) sd_[s] = w.sd[s], nby_[s] = w.nby[s];
    }

    // ---- per-stream state
    const size_t mtb = (size_t) Bpad_ / 16;
    d_hist_[0] = (int16_t *) dalloc((size_t) Bpad_ * kFrame * 2, true);
    d_hist_[1] = (int16_t *) dalloc((size_t) Bpad_ * kFrame * 2, true);
    d_tail_[0] = (float *) dalloc((size_t) Bpad_ * kFrame * 4, true);
    d_tail_[1] = (float *) dalloc((size_t) Bpad_ * kFrame * 4, true);
    d_hstate_[0] = (float *) dalloc((size_t) kGruLayers * mtb * kUnitTiles * 1024, true);
    d_hstate_[1] = (float *) dalloc((size_t) kGruLayers * mtb * kUnitTiles * 1024, true);
    d_hprev_ = dalloc((size_t) kGruLayers * mtb * nbh_ * 1024, true);  // the state in operand form (wavefront calls, frame 0)
    d_rmask_ = (uint8_t *) dalloc((size_t) Bpad_, true);
    if (rate_ != kRate16k) {  // the sample-rate stages: their tables and per-stream state (zeros: a fresh stream)
        rs_taps_[0] = rs_table(rs_stage_in(rate_));
        rs_taps_[1] = rs_table(rs_stage_out(rate_));
        for (int c = 0; c < 2; ++c) {
            d_rs_state_[0][c] = (int16_t *) dalloc((size_t) Bpad_ * rs_in_hist(rate_) * 2, true);
            d_rs_state_[1][c] = (int16_t *) dalloc((size_t) Bpad_ * rs_out_hist(rate_) * 2, true);
        }
    }

    // ---- activation workspace
    const size_t M = mtb * (size_t) Tmax_;  // m-tiles per call
    d_spec_ = (float *) dalloc((size_t) Tmax_ * Bpad_ * 256 * 8, true);
    feat_frame_bytes_ = mtb * nbf_ * 1024;
    d_feat_ = dalloc((M + (size_t) (taps_ - 1) * mtb) * nbf_ * 1024, true);  // [context frames | the call's frames]
    if (taps_ > 1) {
        // taps_ slots: slots 1 .. taps_ - 1 hold the features of the last taps_ - 1 frames; slot 0 is where a one-frame call's roll
        // puts the oldest tap (kns_stft.hip, AnalysisArgs::feat_hist)
        d_fhist_ = dalloc((size_t) taps_ * feat_frame_bytes_, true);
        // one m-tile whose 16 rows are the feature of a silent frame, in the operand type and layout of `feat`: made by the
        // analysis kernel itself from 16 streams of zeros, so that "reset" and "silent frames" are the same bits in both
        // configurations (the bf16 one takes its logarithm from v_log_f32, which no host formula reproduces)
        d_silent_ = dalloc((size_t) nbf_ * 1024, true);
    }
    if (!fold_) d_e_ = dalloc(M * nbh_ * 1024, true);
    for (int s = 0; s < kStages - 1; ++s) d_y_[s] = dalloc(M * nby_[s] * 1024, true);
    d_gi_ = dalloc(M * kGateTiles * 64 * pi_.gisz, true);
    d_hseq_a_ = dalloc(M * nbh_ * 1024, true);
    d_hseq_b_ = dalloc(M * nbh_ * 1024, true);
    d_mask_ = (float *) dalloc(M * kMaskTiles * 1024, true);
    if (!gru_quad_supported(prec_, (int) mtb, 0)) use_quad_ = false;
    if (qdbg_block_ >= 0) d_qdbg_ = (unsigned long long *) dalloc((size_t) 8 * 4 * 8 * 8, true);
    d_in_ = (int16_t *) dalloc((size_t) B_ * Tmax_ * kFrame * 2, true);
    d_out_ = (int16_t *) dalloc((size_t) B_ * Tmax_ * kFrame * 2, true);
    if (alloc_failed_) {
        *oom = true;
        *err = "Failed to allocate device memory.";
        return false;
    }
    if (hipHostMalloc((void **) &h_in_, (size_t) B_ * Tmax_ * kFrame * 2, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **) &h_out_, (size_t) B_ * Tmax_ * kFrame * 2, hipHostMallocDefault) != hipSuccess) {
        (void) hipGetLastError();
        *oom = true;
        *err = "Failed to allocate pinned host memory.";
        return false;
    }
    d_frame_count_ = (unsigned *) dalloc(64, true);
    if (hipHostMalloc((void **) &h_frame_word_, 64, hipHostMallocDefault) != hipSuccess) {
        (void) hipGetLastError();
        h_frame_word_ = nullptr;  // (no completion word: one-frame replays wait in hipStreamSynchronize)
    } else {
        *h_frame_word_ = 0;
    }
    // KOALA_AMD_WAIT=block (product option): one-frame host calls sleep in hipStreamSynchronize instead of polling the frame's
    // completion word -- for hosts that run more streaming handles than they have cores
    {
        const char *w = getenv("KOALA_AMD_WAIT");
        spin_wait_ = dev_env("KOALA_AMD_NO_SPIN_WAIT") == nullptr && !(w && !strcmp(w, "block"));
    }
    if (taps_ > 1) {  // the front-end context of a fresh stream is silence, not zeros
        AnalysisArgs an;
        an.pcm = d_in_;  // zeros (at least one frame of B_ >= 1 streams; rows past the last stream re-read the last one)
        an.hist_in = d_hist_[0];
        an.hist_out = d_hist_[0];  // (zeros over zeros)
        an.window = d_window_;
        an.twiddle = d_twiddle_;
        an.mean = d_mean_;
        an.scale = d_scale_;
        an.spec = nullptr;
        an.feat = d_silent_;
        an.B = 1;
        an.Bpad = 16;
        an.T = 1;
        an.nbf = nbf_;
        an.precision = prec_;
        an.seg = 1;
        an.write_spec = 0;
        launch_analysis(an, own_stream_);
        std::string e2;
        if (!reset(nullptr, &e2)) {
            *err = e2;
            return false;
        }
    }
    if (hipStreamSynchronize(own_stream_) != hipSuccess) {
        *err = std::string("Device initialisation failed: ") + hipGetErrorString(hipGetLastError());
        return false;
    }
    return true;
}

Engine::~Engine() {
    if (own_stream_) (void) hipStreamSynchronize(own_stream_);
    if (copy_out_) (void) hipStreamSynchronize(copy_out_);  // (asynchronous host calls still writing into the caller's buffers)
    for (Span &s : spans_) {
        (void) hipEventDestroy(s.a);
        (void) hipEventDestroy(s.b);
    }
    for (hipEvent_t e : pool_) (void) hipEventDestroy(e);
    for (hipGraphExec_t ge : frame_graph_)
        if (ge) (void) hipGraphExecDestroy(ge);
    for (void *p : allocs_) (void) hipFree(p);
    if (h_frame_word_) (void) hipHostFree(h_frame_word_);
    if (h_in_) (void) hipHostFree(h_in_);
    if (h_out_) (void) hipHostFree(h_out_);
    if (h_report_) (void) hipHostFree(h_report_);
    for (Upload *u : uploads()) u->release();
    for (int i = 0; i < 4; ++i)
        if (aev_out_[i]) (void) hipEventDestroy(aev_out_[i]);
    for (int i = 0; i < 2; ++i) {
        if (aev_in_[i]) (void) hipEventDestroy(aev_in_[i]);
        if (aev_done_[i]) (void) hipEventDestroy(aev_done_[i]);
        if (ev_in_[i]) (void) hipEventDestroy(ev_in_[i]);
        if (ev_done_[i]) (void) hipEventDestroy(ev_done_[i]);
        if (ev_out_[i]) (void) hipEventDestroy(ev_out_[i]);
    }
    for (int i = 0; i < kPipeStreams; ++i) {
        if (pipe_stream_[i]) (void) hipStreamSynchronize(pipe_stream_[i]), (void) hipStreamDestroy(pipe_stream_[i]);
        if (pipe_join_[i]) (void) hipEventDestroy(pipe_join_[i]);
    }
    if (pipe_fork_) (void) hipEventDestroy(pipe_fork_);
    for (int i = 0; i < kPipeRing; ++i)
        if (pipe_syn_[i]) (void) hipEventDestroy(pipe_syn_[i]);
    for (int i = 0; i < kPipeRing; ++i)
        for (int l = 0; l < kGruLayers; ++l)
            if (pipe_ev_[i][l]) (void) hipEventDestroy(pipe_ev_[i][l]);
    if (host_fork_) (void) hipEventDestroy(host_fork_);
    if (copy_in_) (void) hipStreamDestroy(copy_in_);
    if (copy_out_) (void) hipStreamDestroy(copy_out_);
    if (own_stream_) (void) hipStreamDestroy(own_stream_);
}

void Engine::tick(int) {
    if (!profiling_) return;
    hipEvent_t e;
    if (pool_.empty()) {
        (void) hipEventCreate(&e);
    } else {
        e = pool_.back();
        pool_.pop_back();
    }
    (void) hipEventRecord(e, stream_);
    pending_ = e;
}

void Engine::tock(int cls) {
    if (!profiling_) return;
    hipEvent_t e;
    if (pool_.empty()) {
        (void) hipEventCreate(&e);
    } else {
        e = pool_.back();
        pool_.pop_back();
    }
    (void) hipEventRecord(e, stream_);
    spans_.push_back({cls, pending_, e});
}

void Engine::profile_enable(bool on) {
    profiling_ = on;
    if (on) {
        for (int i = 0; i < kNumKernelClasses; ++i) {
            acc_ms_[i] = 0;
            acc_n_[i] = 0;
        }
    }
}

bool Engine::profile_read(double *ms, int64_t *launches, std::string *err) {
    if (hipStreamSynchronize(stream_) != hipSuccess) {
        *err = hip_last_error();
        return false;
    }
    for (Span &s : spans_) {
        float t = 0;
        (void) hipEventElapsedTime(&t, s.a, s.b);
        acc_ms_[s.cls] += t;
        acc_n_[s.cls] += 1;
        pool_.push_back(s.a);
        pool_.push_back(s.b);
    }
    spans_.clear();
    for (int i = 0; i < kNumKernelClasses; ++i) {
        ms[i] = acc_ms_[i];
        launches[i] = acc_n_[i];
    }
    return true;
}

bool Engine::synchronize(std::string *err) {
    if (async_n_ && !drain_async(err)) return false;
    if (hipStreamSynchronize(stream_) != hipSuccess) {
        *err = hip_last_error();
        return false;
    }
    return true;
}

ResetArgs Engine::reset_args(const uint8_t *d_mask) const {
    ResetArgs r;
    r.hist = d_hist_[0];
    r.hist2 = d_hist_[1];
    r.tail = d_tail_[0];
    r.tail2 = d_tail_[1];
    r.hstate = d_hstate_[0];
    r.hstate2 = d_hstate_[1];
    r.Bpad = Bpad_;
    r.fhist = d_fhist_;
    r.silent = d_silent_;
    r.fhist_frames = taps_ > 1 ? taps_ : 0;
    r.nbf = nbf_;
    r.mask = d_mask;
    return r;
}

bool Engine::reset(const uint8_t *host_mask, std::string *err) {
    (void) hipSetDevice(device_);
    // (the reset kernel is ordered behind every enqueued call on the handle's stream; nothing to drain)
    ResetArgs r = reset_args(nullptr);
    if (host_mask) {
        std::vector<uint8_t> m((size_t) Bpad_, 0);
        memcpy(m.data(), host_mask, (size_t) B_);
        hipError_t ce = hipMemcpyAsync(d_rmask_, m.data(), (size_t) Bpad_, hipMemcpyHostToDevice, stream_);
        if (ce == hipSuccess) ce = hipStreamSynchronize(stream_);  // `m` goes out of scope
        if (ce != hipSuccess) {  // a stale mask would reset the wrong streams: report, do not launch
            (void) hipGetLastError();
            *err = hip_error(ce);
            return false;
        }
        r.mask = d_rmask_;
    }
    launch_resets(r.mask);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return false;
    }
    for (int b = 0; pk_max_ && b < B_; ++b)
        if (!host_mask || host_mask[b]) pk_fill_[b] = 0;
    for (int b = 0; fr_rate_ && b < B_; ++b)
        if (!host_mask || host_mask[b]) fr_phase_[b] = 0;
    return true;
}

void Engine::launch_resets(const uint8_t *d_mask) {
    launch_reset(reset_args(d_mask), stream_);
    if (rate_ != kRate16k) {
        launch_resample_reset(d_rs_state_[0][0], d_rs_state_[0][1], rs_in_hist(rate_), d_mask, Bpad_, stream_);
        launch_resample_reset(d_rs_state_[1][0], d_rs_state_[1][1], rs_out_hist(rate_), d_mask, Bpad_, stream_);
        if (d_hb_rep_) launch_high_band_reset(d_hb_x_, d_hb_y_, d_hb_s_, rs_stage_out(rate_).U, d_mask, Bpad_, stream_);  // (the high-band carry's, once it exists)
    }
    if (d_lv_state_) launch_level_reset(d_lv_state_, d_mask, Bpad_, stream_);  // (the leveller's, once it exists)
    if (d_lm_state_) launch_limit_reset(d_lm_state_, d_mask, Bpad_, stream_);  // (the limiter's, once it exists)
    if (d_cf_state_) launch_comfort_reset(d_cf_state_, d_mask, Bpad_, stream_);  // (the comfort noise's counters, once they exist)
    if (pk_max_) launch_packet_reset(packet_state_args(), d_mask, stream_);
    if (fr_rate_) launch_fractional_reset(fractional_state_args(), d_mask, stream_);
}

bool Engine::Upload::ready(Engine *e, size_t bytes, bool zero) {
    if (d) return true;
    const bool pinned = host[0] != nullptr;  // (the ring of an earlier try whose dalloc failed)
    bool ok = true;
    for (int i = 0; i < kUploadRing && ok && !pinned; ++i)
        ok = hipHostMalloc(&host[i], bytes, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void) hipGetLastError();
        release();
        return false;
    }
    d = e->dalloc(bytes, zero);
    return d != nullptr;
}

void *Engine::Upload::take(int *slot) {
    const int k = (int) (n % kUploadRing);
    if (pending[k] && hipEventSynchronize(ev[k]) != hipSuccess) return nullptr;
    pending[k] = false;
    ++n;
    *slot = k;
    return host[k];
}

bool Engine::Upload::send(int slot, size_t bytes, hipStream_t stream, void *to) {
    pending[slot] = hipMemcpyAsync(to ? to : d, host[slot], bytes, hipMemcpyHostToDevice, stream) == hipSuccess &&
                    hipEventRecord(ev[slot], stream) == hipSuccess;
    return pending[slot];
}

void Engine::Upload::release() {
    for (int i = 0; i < kUploadRing; ++i) {
        if (host[i]) (void) hipHostFree(host[i]);
        if (ev[i]) (void) hipEventDestroy(ev[i]);
        host[i] = nullptr;
        ev[i] = nullptr;
        pending[i] = false;
    }
}

// Per-frame stream resets of the call about to run (Call::resets, uint8 [B][T] host memory), before anything of the call is enqueued
// (begin_call); `table` is the setup's, fresh.  Resets at frame 0 only: the reset kernel in front of the call, which then takes its normal route.
// Resets at some frame t > 0 (refused for a several-frame front-end, whose feature history the reset arms do not rebuild): the mask is
// packed per (m-tile, frame) into a slot of rs_up_ -- bit r of word [mt][t] = stream 16 mt + r restarts right before frame t -- and
// `table` says so; run_device sends the slot on the stream of the call's kernels and reads the table through the kernels' reset arms
// (kRouteChunkedResets).  A slot is as large as the larger of the two things it may carry, the table and the frame-0 mask.
bool Engine::begin_resets(int T, const uint8_t *mask, ResetTable *table, std::string *err) {
    if (!mask) return true;
    bool first = false, late = false;
    for (int b = 0; b < B_; ++b) {
        const uint8_t *row = mask + (size_t) b * T;
        first = first || row[0];
        for (int t = 1; t < T && !late; ++t) late = row[t] != 0;
    }
    if (!first && !late) return true;  // (an all-zero mask: the plain call, same route and bits)
    if (late && taps_ > 1) {
        *err = "per-frame stream resets after frame 0 are not supported for models with a several-frame front-end (front_taps > 1).";
        return false;
    }
    const int mtb = Bpad_ / 16;
    if (!rs_up_.ready(this, std::max((size_t) mtb * Tmax_ * 4, (size_t) Bpad_))) {
        *err = "Failed to allocate the buffers of per-frame stream resets.";
        return false;
    }
    int k;
    void *slot = rs_up_.take(&k);
    if (!slot) {
        *err = hip_last_error();
        return false;
    }
    if (!late) {  // frame 0 only: the reset kernel on the call's stream, right in front of it
        uint8_t *bytes = (uint8_t *) slot;
        memset(bytes, 0, (size_t) Bpad_);
        for (int b = 0; b < B_; ++b) bytes[b] = mask[(size_t) b * T] != 0;
        const bool ok = rs_up_.send(k, (size_t) Bpad_, stream_, d_rmask_);
        if (ok) launch_reset(reset_args(d_rmask_), stream_);
        const hipError_t e = hipGetLastError();
        if (!ok || e != hipSuccess) {
            *err = hip_error(e);
            return false;
        }
        return true;
    }
    unsigned *w = (unsigned *) slot;
    memset(w, 0, (size_t) mtb * T * 4);
    table->frame.assign((size_t) T, 0);
    for (int b = 0; b < B_; ++b) {
        const uint8_t *row = mask + (size_t) b * T;
        unsigned *wm = w + (size_t) (b >> 4) * T;
        const unsigned bit = 1u << (b & 15);
        for (int t = 0; t < T; ++t)
            if (row[t]) {
                wm[t] |= bit;
                table->frame[t] = 1;
            }
    }
    table->slot = k;
    table->T = T;
    return true;
}

// A per-stream setting of the call about to run (`rows`: host memory, B rows of `row` bytes), before anything of the call is enqueued and
// outside any capture.  When the call's revision is not the one the device table holds, the rows go (rows past B: zero) to the device on
// the handle's stream, where every kernel of the previous call is in front of the copy -- a call in flight keeps the setting it was issued
// under -- and every kernel of this one behind it; an unchanged setting costs a call nothing.  The caller's rows have been read when this
// returns.
bool Engine::put_table(SettingTable *t, size_t row, const void *rows, unsigned rev, const char *what, std::string *err) {
    if (!table_alloc(t, row)) {
        (void) hipGetLastError();
        *err = std::string("Failed to allocate the buffers of ") + what + ".";
        return false;
    }
    if (t->valid && t->rev == rev) return true;
    int k;
    char *slot = (char *) t->up.take(&k);
    if (slot) {
        memcpy(slot, rows, (size_t) B_ * row);
        memset(slot + (size_t) B_ * row, 0, (size_t) (Bpad_ - B_) * row);
    }
    if (!slot || !t->up.send(k, (size_t) Bpad_ * row, stream_)) {
        *err = hip_last_error();
        t->valid = false;
        return false;
    }
    t->rev = rev;
    t->valid = true;
    return true;
}

const Engine::OutputStage (&Engine::output_stages())[3] {
    static const OutputStage stages[3] = {
        {kStageLevel, "the output leveller", "a levelling call", "the output leveller", false, &Engine::level_ready, &StreamOptions::level_rev,
         {{&Engine::lv_tab_, sizeof(LevelSetting), [](const StreamOptions &o) -> const void * { return o.level; }}, {}}},
        {kStageLimiter, "the peak limiter", "a limiting call", "the peak limiter", false, &Engine::limiter_ready, &StreamOptions::limiter_rev,
         {{&Engine::lm_tab_, sizeof(LimiterSetting), [](const StreamOptions &o) -> const void * { return o.limiter; }}, {}}},
        {kStageComfort, "comfort noise", "a call with comfort noise", "the comfort noise", true, &Engine::comfort_ready, &StreamOptions::comfort_rev,
         {{&Engine::cf_tab_, sizeof(ComfortSetting), [](const StreamOptions &o) -> const void * { return o.comfort; }},
          {&Engine::cfa_tab_, (size_t) kComfortRow * 4, [](const StreamOptions &o) -> const void * { return o.comfort_amp; }}}},
    };
    return stages;
}

bool Engine::refuse_stages(const StreamOptions &o, const char *why, std::string *err) {
    for (const OutputStage &s : output_stages())
        if (s.on(o)) {
            *err = std::string(s.name) + why;
            return true;
        }
    return false;
}

bool Engine::begin_call(const Call &c, bool device_rows, CallSetup *cs, std::string *err) {
    const StreamOptions &o = c.opt;
    if (o.band_profile && (o.channel_link || c.high_band || !o.min_gain)) {
        *err = !o.min_gain ? "a call with a band profile carries the handle's minimum gains (all zero where no limit is in force)."
                           : "a band profile is not combined with linked channels nor with the high-band carry.";
        return false;
    }
    // (linked channels and output stages: process() hands such a call on with device rows, so the host routes, the one-frame graph among
    // them, never see one: never quietly unlinked or without a stage.  Comfort noise: its kernels carry the gains and the profile's clamp)
    cs->link = o.channel_link ? ch_ : 0;
    if (cs->link && (!o.min_gain || !device_rows)) {
        *err = !o.min_gain ? "a linked call carries the handle's minimum gains." : "a linked call runs on device rows only.";
        return false;
    }
    for (const OutputStage &s : output_stages()) {
        if (!s.on(o)) continue;
        cs->stages |= s.bit;
        if (!device_rows || (s.carries_profile && !o.band_profile) || cs->link || c.high_band) {
            *err = !device_rows                          ? std::string(s.call) + " runs on device rows only." :
                   s.carries_profile && !o.band_profile ? std::string(s.call) + " carries the handle's band profile (neutral where none is in force)." :
                                                          std::string(s.name) + " is not combined with linked channels nor with the high-band carry.";
            return false;
        }
    }
    // (the reset mask, the gains and the profile are copied into upload slots of this call: the caller may overwrite them when this returns)
    if (!begin_resets(c.T, c.resets, &cs->resets, err)) return false;
    if (o.min_gain && !put_table(&mg_tab_, 4, o.min_gain, o.min_gain_rev, "the per-stream attenuation limit", err)) return false;
    if (o.band_profile && !put_table(&pf_tab_, (size_t) kProfileRow * 4, o.band_profile, o.band_profile_rev, "the band profile", err)) return false;
    cs->min_gain = o.min_gain ? (const float *) mg_tab_.up.d : nullptr;
    cs->profile = o.band_profile ? (const float *) pf_tab_.up.d : nullptr;
    for (const OutputStage &s : output_stages()) {
        if (!(cs->stages & s.bit)) continue;
        if (!(this->*s.ready)(err)) return false;
        for (const OutputStage::Table &t : s.table)
            if (t.tab && !put_table(&(this->*t.tab), t.row, t.rows(o), o.*s.rev, s.what, err)) return false;
    }
    if (cs->stages & kStageComfort) cs->comfort_set = (const ComfortSetting *) cf_tab_.up.d, cs->comfort_amp = (const float *) cfa_tab_.up.d;
    return !cs->stages || control_rows(c, &cs->ctl, err);
}

// The staging of the frame report of host-pointer calls, before anything of the call is enqueued and outside any capture.
bool Engine::report_ready(bool second_slot, std::string *err) {
    const size_t bytes = (size_t) B_ * Tmax_ * 16;
    if (!d_report_) d_report_ = (float *) dalloc(bytes, true);
    if (d_report_ && !h_report_ && hipHostMalloc((void **) &h_report_, bytes, hipHostMallocDefault) != hipSuccess) h_report_ = nullptr;
    if (second_slot && !d_report2_) d_report2_ = (float *) dalloc(bytes, true);
    if (!d_report_ || !h_report_ || (second_slot && !d_report2_)) {
        (void) hipGetLastError();
        *err = "Failed to allocate the staging buffers of the frame report.";
        return false;
    }
    return true;
}

// the arguments of one GRU layer of ONE frame (frame t of a call) for the low-latency layer kernel and the wavefront's items
GruSmallArgs Engine::small_args(int mtb, const void *a0, int nb0, const void *a1, const void *wih, const float *bih, const void *whh,
                                const float *bhh, int layer, void *hseq, int t, const StageDev *head) const {
    GruSmallArgs g;
    const size_t frame = (size_t) t * mtb * 1024;  // bytes of one k-block column of A per frame
    if (head) {  // the narrow head of the stage before, inside this launch
        g.yh = (const char *) d_hseq_b_ + frame * nbh_;
        g.yw = head->w_head;
        g.yb = head->b_head;
        g.yvalid = head->head_dim;
    }
    g.a0 = a0 ? (const char *) a0 + frame * nb0 : nullptr;
    g.a1 = (const char *) a1 + frame * nbh_;
    g.wih = wih;
    g.bih = bih;
    g.whh = whh;
    g.bhh = bhh;
    g.hstate_in = d_hstate_[(hs_cur_ + t) & 1] + (size_t) layer * mtb * kUnitTiles * 256;
    g.hstate_out = d_hstate_[(hs_cur_ + t + 1) & 1] + (size_t) layer * mtb * kUnitTiles * 256;
    g.hseq = (char *) hseq + frame * nbh_;
    g.nb0 = nb0;
    g.mtiles = mtb;
    g.precision = prec_;
    return g;
}

// ---- calls of several frames as a WAVEFRONT over (pipeline stage, frame): the stages are the eight GRU layers with the three narrow
// heads between them; stage i of frame t needs stage i - 1 of frame t and (a layer) its own frame t - 1, so launch k runs the items with
// i + t = k side by side (kns_gru.hip, gru_wave_kernel) -- T + 10 launches of up to 8 x 17 x groups workgroups instead of 8 T launches of
// 17 x mtb (kRouteSmallSteps) or of mtb (the chunked recurrent kernels).  The per-frame slots of the two hidden-sequence buffers, of the
// y operands and of the features' padding are reused stage after stage exactly as in the layer-by-layer order: within a frame the stages
// still run one after the other.
GruWaveItem Engine::wave_item(int i, int t, int mtb) const {  // stage i (layers 3 s, 3 s + 1; head 3 s + 2) of frame t
    const int s = i / 3, r = i % 3;
    const StageDev &d = sd_[s];
    const size_t frame = (size_t) t * mtb * 1024;
    char *feat_call = (char *) d_feat_ + (size_t) (taps_ - 1) * feat_frame_bytes_;
    GruWaveItem it;
    if (r == 2) {  // the head of stage s
        it.g.yh = (const char *) d_hseq_b_ + frame * nbh_;
        it.g.yw = d.w_head;
        it.g.yb = d.b_head;
        it.g.yvalid = d.head_dim;
        it.g.mtiles = mtb;
        it.g.precision = prec_;
        if (sd_[s + 1].ypad) {  // into columns 257 ... of the features (k = 1 ... of their block 8)
            it.chains = 1;
            it.pad = 1;
            it.yout = feat_call + frame * nbf_;
            it.y_nb = nbf_;
            it.y_blk = kBins / pi_.kb;
            it.y_kk0 = kBins % pi_.kb;
        } else {
            it.chains = d.head_tiles;
            it.yout = (char *) d_y_[s] + frame * nby_[s];
            it.y_nb = nby_[s];
        }
        return it;
    }
    // h_{t-1} in operand form: the layer's hidden-sequence slot of the frame before, or the converted state (d_hprev_) for frame 0
    const void *hseq = r ? d_hseq_b_ : d_hseq_a_;
    it.hprev = t ? (const char *) hseq + (frame - (size_t) mtb * 1024) * nbh_ : (const char *) d_hprev_ + (size_t) (2 * s + r) * mtb * nbh_ * 1024;
    if (r == 1) {
        it.g = small_args(mtb, nullptr, 0, d_hseq_a_, d.w_ih_b, d.b_ih_b, d.w_hh_b, d.b_hh_b, 2 * s + 1, d_hseq_b_, t, nullptr);
    } else {
        const bool y = s && !d.ypad;
        it.g = small_args(mtb, y ? d_y_[s - 1] : nullptr, y ? nby_[s - 1] : 0, fold_ ? (const void *) feat_call : (const void *) d_e_, d.w_ih_a,
                          d.b_ih_a, d.w_hh_a, d.b_hh_a, 2 * s, d_hseq_a_, t, nullptr);
    }
    return it;
}

bool Engine::wave_fits() const {  // every head either goes into the features' padding or is a y operand of 1-3 k-blocks
    for (int s = 0; s < kStages - 1; ++s)
        if (!(sd_[s + 1].ypad ? sd_[s].head_dim <= 16 : (nby_[s] >= 1 && nby_[s] <= 3 && sd_[s].head_tiles == pi_.npb * nby_[s]))) return false;
    return true;
}

// streams and events of the layer pipeline (run_device), made on first use
bool Engine::pipe_ready() {
    if (pipe_ok_) return true;
    if (pipe_failed_) return false;
    bool ok = true;
    for (int i = 0; i < kPipeStreams && ok; ++i) {
        if (!pipe_stream_[i]) ok = hipStreamCreateWithFlags(&pipe_stream_[i], hipStreamNonBlocking) == hipSuccess;
        if (ok && !pipe_join_[i]) ok = hipEventCreateWithFlags(&pipe_join_[i], hipEventDisableTiming) == hipSuccess;
    }
    if (ok && !pipe_fork_) ok = hipEventCreateWithFlags(&pipe_fork_, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < kPipeRing && ok; ++i)
        for (int l = 0; l < kGruLayers && ok; ++l)
            if (!pipe_ev_[i][l]) ok = hipEventCreateWithFlags(&pipe_ev_[i][l], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < kPipeRing && ok; ++i)
        if (!pipe_syn_[i]) ok = hipEventCreateWithFlags(&pipe_syn_[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void) hipGetLastError();
        pipe_failed_ = true;  // (the plain chunked route stays)
        return false;
    }
    pipe_ok_ = true;
    return true;
}

void Engine::run_wave(int T, int mtb) {
    // m-tiles per workgroup (an XCD holds 64 workgroups at a time, a layer has 17 per group; measured best: 1 up to 64 streams,
    // 3 up to 256 (fp32: 512), then 6 in bf16, 4 up to 2 048 and 8 beyond in fp32 -- short groups balance the CUs, long ones pull the
    // weights less often; within ~3 % of the best of {1, 2, 3, 4, 6, 8} at every size swept, profiles/r04_wavefront.txt)
    int mgroup = mtb <= 4 ? 1 : prec_ == kBf16 ? (mtb <= 16 ? 3 : 6) : (mtb <= 32 ? 3 : mtb <= 128 ? 4 : 8);
    if (dev_wave_group_ > 0) mgroup = dev_wave_group_;
    tick(kClsGru);
    launch_gru_wave_prev(d_hstate_[hs_cur_], d_hprev_, kGruLayers * mtb, prec_, stream_);
    tock(kClsGru);
    for (int k = 0; k < T + kWaveItems - 1; ++k) {
        GruWaveArgs w;
        w.mgroup = mgroup;
#ifdef KNS_TIMING
        w.stamp = k == T / 2 + 5;
#endif
        w.layer_wgs = kUnitTiles * ((mtb + mgroup - 1) / mgroup);
        for (int x = 0; x < 8; ++x) w.layer_item[x] = w.head_item[x] = -1, w.layer_part[x] = 0;
        int n = 0, layers = 0;
        const int i0 = k < T ? 0 : k - T + 1;
        for (int i = i0; i <= k && i < kWaveItems; ++i) layers += i % 3 != 2;
        // one layer per XCD; four or fewer layers (the pipeline filling or draining) take 2, 4 or 8 XCDs each
        w.parts = dev_wave_parts_ ? (layers <= 1 ? 8 : layers <= 2 ? 4 : layers <= 4 ? 2 : 1) : 1;
        w.xcd_wgs = (w.layer_wgs + w.parts - 1) / w.parts;
        int seen = 0;
        for (int i = i0; i <= k && i < kWaveItems; ++i) {
            w.item[n] = wave_item(i, k - i, mtb);
            if (i % 3 == 2) {  // the head of stage s: beside a layer's workgroups, on the XCD(s) of the layer before it in this launch
                w.head_item[w.parts == 1 ? 2 * (i / 3) + 1 : (seen ? seen - 1 : 0) * w.parts] = n;
            } else {
                for (int q = 0; q < w.parts; ++q) {
                    const int x = w.parts == 1 ? 2 * (i / 3) + i % 3 : seen * w.parts + q;  // (all eight in flight: layer l on XCD l)
                    w.layer_item[x] = n;
                    w.layer_part[x] = q;
                }
                ++seen;
            }
            ++n;
        }
        tick(kClsGru);
        launch_gru_wave(w, prec_, mtb, stream_);
        tock(kClsGru);
    }
}

// ---- dispatch: which kernel family a call takes (mtb = m-tiles of 16 streams = ceil(B / 16); edges measured on MI355X, each
// tested from both sides by tests/test_gpu_parity.py::test_dispatch_boundaries; the developer build reports the route of the
// last call through debug tap 6, tests/test_gpu_parity.py::test_dispatch_routes)
//
//   GRU layers (8 per call)
//   | configuration | frames T | m-tiles mtb                           | route                                                        |
//   |---------------|----------|---------------------------------------|--------------------------------------------------------------|
//   | bf16          | 1        | <= 59, or not whole quads up to 192   | kRouteSmall: gru_small_kernel, one launch per layer           |
//   | bf16          | 1        | >= 60 and mtb % 4 == 0                | kRouteQuad1: gru_quad1_kernel, one launch per layer; stage    |
//   |               |          |                                       |   inputs wider than 2 k-blocks: input GEMM + recurrent kernel |
//   | bf16          | 1        | > 192 and mtb % 4 != 0                | kRouteChunked                                                 |
//   | bf16          | > 1      | <= 48 (<= 64 up to T = 4)             | kRouteWave: gru_wave_kernel, T + 10 launches: the (stage,     |
//   |               |          |                                       |   frame) items of one anti-diagonal side by side, one layer   |
//   |               |          |                                       |   per XCD, narrow heads as items of their own                 |
//   | bf16          | >= 32    | 49 .. 144                             | kRoutePipelined: the chunked kernels on TWO sub-chunks of     |
//   |               |          |                                       |   frames, the (layer, sub-chunk) grid as a wavefront over two |
//   |               |          |                                       |   streams; >= 48 frames and <= 112 m-tiles: analysis and      |
//   |               |          |                                       |   synthesis per sub-chunk too                                 |
//   | bf16          | > 1      | otherwise                             | kRouteChunked: gemm_ws2 (m-tiles in multiples of 256 x stage; |
//   |               |          |                                       |   the rest through gemm_kernel) + gru_resident8_kernel        |
//   | fp32          | 1        | <= 256                                | kRouteSmall                                                   |
//   | fp32          | 1        | > 256                                 | kRouteChunked: gemm_kernel + gru_kernel<PF32, 8>              |
//   | fp32          | > 1      | <= 256                                | kRouteWave                                                   |
//   | fp32          | > 1      | <= 192, wavefront off (developer      | kRouteSmallSteps: gru_small_kernel frame by frame (T launches |
//   |               |          |   switch, debug taps)                 |                                                              |
//   |               |          |                                       |   per layer; the chunked recurrence would occupy mtb CUs)     |
//   | fp32          | > 1      | > 192                                 | kRouteChunked                                                 |
//   | both          | any      | any: a call (host-pointer calls: a    | kRouteChunkedResets: the chunked kernels' reset arms          |
//   |               |          |   sub-chunk) with per-frame stream    |   (analysis_kernel, synthesis_kernel, gru_resident8_kernel /  |
//   |               |          |   resets at some frame t > 0 (t = 0   |   gru_kernel<PF32, 8>: kResets) read the rows that restart    |
//   |               |          |   only: reset kernel + normal route)  |   per (m-tile, frame); GEMMs and heads unchanged; developer   |
//   |               |          |                                       |   A/B switches of the recurrent kernel not honoured           |
//
//   Around them (all configurations)
//   | what                          | T = 1, bf16                                         | otherwise                            |
//   |-------------------------------|-----------------------------------------------------|--------------------------------------|
//   | spectrum                      | stored by analysis, read by synthesis (in place)    | T > 1: rebuilt from the PCM by the   |
//   |                               |                                                     | synthesis kernel (not if in == out)  |
//   | front-end GEMM                | none: folded into the stage-input GEMMs (one-frame  | bf16, T > 1: none either; fp32 and   |
//   |                               | front-end); five-frame: gemm_front5_t1_kernel       | KNS-v1.1: gemm_wsr / front5 / generic |
//   | narrow heads 1 / 5 / 40       | inside the next stage's first layer launch          | wavefront: items of their own; bf16  |
//   |                               |                                                     | chunked: 1 and 5 inside their        |
//   |                               |                                                     | layer-B recurrent launch; gemm_head  |
//   | mask head                     | inside the synthesis launch                         | gemm_wsr_kernel                      |
//   | analysis / synthesis segments | one                                                 | ~4 / ~2 workgroups per CU (>= 1 frame)  |
//   Host-pointer calls: >= 4 MiB and more than min(16, max_frames / 2) frames -> sub-chunks on three streams; T = 1 -> hipGraph replay.
enum Route { kRouteChunked = 0, kRouteSmall = 1, kRouteSmallSteps = 2, kRouteQuad1 = 3, kRouteWave = 4, kRoutePipelined = 5, kRouteChunkedResets = 6 };

bool Engine::run_device(const Slice &slice, std::string *err) {
    const int T = slice.T;
    const int16_t *d_pcm = slice.d_pcm;
    int16_t *d_out = slice.d_out;
    const bool allow_recompute = slice.allow_recompute;
    const int mtb = Bpad_ / 16;
    last_T_ = T;
    // per-frame stream resets in these frames (begin_resets): the chunked route with the kernels' reset arms, whatever the batch size
    ResetTable *table = !slice.without_reset_table && slice.call->resets.slot >= 0 ? &slice.call->resets : nullptr;
    const bool resets = table && std::any_of(table->frame.begin() + slice.t0, table->frame.begin() + slice.t0 + T, [](uint8_t v) { return v != 0; });
    if (resets && !table->uploaded) {  // the call's table, on the stream of its kernels (its first sub-chunk that needs it)
        (void) rs_up_.send(table->slot, (size_t) mtb * table->T * 4, stream_);
        table->uploaded = true;
    }
    const unsigned *rs = resets ? (const unsigned *) rs_up_.d : nullptr;
    const int rs_pitch = table ? table->T : 0, rs_t0 = slice.t0;  // (where these frames are in the table)

    AnalysisArgs an;
    an.pcm = d_pcm;
    // T == 1: the one workgroup that reads a stream's history also writes it (same lanes, same addresses), so the state
    // is updated in place and the launch arguments never change -- which is what lets the frame be a hipGraph
    const bool in_place = T == 1;
    an.hist_in = d_hist_[hist_cur_];
    an.hist_out = d_hist_[in_place ? hist_cur_ : hist_cur_ ^ 1];
    an.window = d_window_;
    an.twiddle = d_twiddle_;
    an.mean = d_mean_;
    an.scale = d_scale_;
    an.spec = d_spec_;
    char *feat_now = (char *) d_feat_ + (size_t) (taps_ - 1) * feat_frame_bytes_;  // behind the context frames
    an.feat = feat_now;
    char *fhist_last = (char *) d_fhist_ + feat_frame_bytes_;  // the last taps_ - 1 frames' features
    // one-frame calls of a several-frame front-end: the analysis kernel rolls the history itself and writes the frame's features
    // into its last slot; the front-end reads its taps from there (no copy launches)
    const bool roll_in_analysis = taps_ > 1 && T == 1 && fuse_front_ && !debug_taps_;
    if (roll_in_analysis) {
        an.feat_hist = d_fhist_;
        an.hist_slots = taps_ - 1;
        an.feat = (char *) d_fhist_ + (size_t) (taps_ - 1) * feat_frame_bytes_;
    } else if (taps_ > 1) {  // [features of the last taps - 1 frames | this call's]: the front-end reads taps shifted views of it
        (void) hipMemcpyAsync(d_feat_, fhist_last, (size_t) (taps_ - 1) * feat_frame_bytes_, hipMemcpyDeviceToDevice, stream_);
    }
    an.B = B_;
    an.Bpad = Bpad_;
    an.T = T;
    an.nbf = nbf_;
    an.precision = prec_;
    an.resets = rs;
    an.rs_pitch = rs_pitch;
    an.rs_t0 = rs_t0;
    // The spectrum makes its round trip through HBM only where it has to: in single-frame calls (the history is updated in
    // place there, so the synthesis kernel cannot rebuild it) and when the debug taps are on.  Otherwise the synthesis
    // kernel recomputes it from the PCM.
    // (a caller whose `enhanced` overlaps its `pcm` gets the stored-spectrum form: the synthesis kernel would otherwise
    // read input frames it has already overwritten)
    const bool recompute = !in_place && !no_recompute_ && allow_recompute;
    an.write_spec = !recompute || debug_taps_;
    spec_valid_ = an.write_spec != 0;
    {   // time segments: about four workgroups per CU
        const int seg_env = dev_analysis_seg_;
        int seg = T;
        // (down to one frame per workgroup for few streams: 16 streams x 32 frames, whole call, 0.216 -> 0.192 ms)
        while (seg > 1 && (Bpad_ / 16) * ((T + seg - 1) / seg) < 1024) seg = (seg + 1) / 2;
        an.seg = seg_env > 0 ? (seg_env < T ? seg_env : T) : seg;
    }
    feat_valid_ = !roll_in_analysis;  // (otherwise the features went to the history slots)
    const int16_t *hist_before = d_hist_[hist_cur_];
    const int only = dev_only_class_;  // -1 in the product library
    // (the analysis launch itself follows the route decisions below: the layer pipeline of mid-size batches cuts it into slices of frames)

    // Time slice of the call the launches below work on, and where they go: the whole call on the handle's stream -- or, for mid-size
    // batches, one of its sub-chunks on one of the pipeline streams (run_pipelined below).  Every activation matrix is frame-major
    // ([frame][m-tile][blocks]), so a slice of frames is a contiguous slice of each of them.
    int c_t0 = 0, c_T = T, c_hs = hs_cur_, c_grid = 0;
    hipStream_t c_stream = stream_;
    auto gemm = [&](int cls, const void *a0, int nb0, const void *a1, int nb1, const void *w, const float *bias,
                    void *out, int ntiles, int n_valid, int kind, int taps = 1, int pad_nb = 0, int pad_blk = 0, int pad_kk0 = 0) {
        GemmArgs g;
        g.pad_nb = pad_nb;
        g.pad_blk = pad_blk;
        g.pad_kk0 = pad_kk0;
        g.taps = taps;
        g.tap_stride = feat_frame_bytes_;
        const size_t m0 = (size_t) c_t0 * mtb;  // first m-tile of the slice
        const size_t out_stride = kind == kOutGi ? (size_t) kGateTiles * 64 * pi_.gisz
                                  : kind == kOutMask ? (size_t) kMaskTiles * 256 * (prec_ == kBf16 ? 2 : 4)
                                                     : (size_t) (pad_nb ? pad_nb : (ntiles + pi_.npb - 1) / pi_.npb) * 1024;
        g.a0 = a0 ? (const char *) a0 + m0 * nb0 * 1024 : nullptr;
        g.a1 = (const char *) a1 + m0 * nb1 * 1024;
        g.w = w;
        g.bias = bias;
        g.out = (char *) out + m0 * out_stride;
        g.nb0 = nb0;
        g.nb1 = nb1;
        g.mtiles = mtb * c_T;
        g.ntiles = ntiles;
        g.n_valid = n_valid;
        g.out_kind = kind;
        g.precision = prec_;
        g.dev = dev_variant_;
        g.grid = c_grid;
        tick(cls);
        if (only < 0 || only == cls) launch_gemm(g, c_stream);
        tock(cls);
    };
    auto gru = [&](const void *whh, const float *bhh, int layer, void *hseq, const StageDev *head = nullptr) {
        GruArgs g;
        const size_t m0 = (size_t) c_t0 * mtb;
        if (head) {  // this stage's narrow head inside the launch, into the padding of the feature matrix (kns_kernels.h)
            ++last_head_launches_;
            g.yw = head->w_head;
            g.yb = head->b_head;
            g.yout = feat_now + (size_t) c_t0 * feat_frame_bytes_;
            g.yvalid = head->head_dim;
            g.y_nb = nbf_;
            g.y_blk = kBins / pi_.kb;
            g.y_kk0 = kBins % pi_.kb;
        }
        g.gi = (const char *) d_gi_ + m0 * kGateTiles * 64 * pi_.gisz;
        g.whh = whh;
        g.bhh = bhh;
        g.hstate_in = d_hstate_[c_hs] + (size_t) layer * mtb * kUnitTiles * 256;
        g.hstate_out = d_hstate_[c_hs ^ 1] + (size_t) layer * mtb * kUnitTiles * 256;
        g.hseq = (char *) hseq + m0 * nbh_ * 1024;  // (left untouched by a launch that carries the head: the head was its only reader)
        g.T = c_T;
        g.mtiles = mtb;
        g.precision = prec_;
        g.dev = dev_variant_;
        g.resets = rs;
        g.rs_pitch = rs_pitch;
        g.rs_t0 = rs_t0;
        tick(kClsGru);
        if (only < 0 || only == kClsGru) launch_gru(g, c_stream);
        tock(kClsGru);
    };

    // One frame per call: whole GRU layers (input GEMM + recurrent GEMM + gates) as single wide launches of the low-latency
    // kernel -- 17 x mtb workgroups that stream their share of both weight matrices from L2, no pre-activation round trip,
    // half the launches.  The weight-resident kernels first pull 459 KiB per CU for ONE step, so the fused form wins up to
    // 192 m-tiles in bf16 (3 072 streams: 218 vs 264 us per frame step; 512 streams: 113 vs 212; at 4 096 it loses, 256 vs
    // 222) and at every size measured in fp32 (4 096 streams: 628 vs 815 us).  Same arithmetic, bit for bit.
    const int small_env = dev_small_mt_;
    // (bf16, m-tiles in whole quads: from 60 m-tiles on the one-step quad kernel is faster -- it takes ~94 us per frame step from
    // 512 to 1 536 streams, 96 at 2 048, 106 at 4 096 (222 with the chunked kernels); the low-latency kernel below 79 us at 512
    // streams, 81 at 704, 99 at 1 024, 120 at 1 536)
    const int small_mt = small_env > 0 ? small_env : (prec_ == kBf16 ? (use_quad_ ? 59 : 192) : 256);
    const bool small = T == 1 && mtb <= small_mt && !no_small_ && !resets;
    // Fewer than 256 m-tiles: the chunked recurrent kernels would occupy mtb workgroups, so the layers run frame
    // by frame through the low-latency kernel instead (17 x mtb workgroups of three waves per frame, input GEMM included):
    // in fp32 at 256 streams x 32 frames 8 x 32 launches of ~13 us beat 8 x (0.1 + 0.75) ms (2.8 vs 1.2 M frames/s; 5.5 vs
    // 3.7 M at 1024 streams, 7.2 vs 6.7 M at 3072, equal at 4096).  Frame t of a call reads the hidden
    // state from ping-pong buffer (hs_cur_ + t) & 1 and writes the other one.
    const int steps_mt = dev_steps_mt_;
    // (fp32 only: the bf16 recurrent kernel keeps its weights on chip and is faster than 8 us per frame and layer even
    // with 16 workgroups -- 11.3 vs 5.2 M frames/s at 256 streams; the fp32 one streams them: 1.2 vs 2.8 M)
    auto gru_small = [&](const void *a0, int nb0, const void *a1, const void *wih, const float *bih, const void *whh,
                         const float *bhh, int layer, void *hseq, int t = 0, const StageDev *head = nullptr) {
        const GruSmallArgs g = small_args(mtb, a0, nb0, a1, wih, bih, whh, bhh, layer, hseq, t, head);
        tick(kClsGru);
        launch_gru_small(g, stream_);
        tock(kClsGru);
    };
    // Where it wins (measured against the other routes, tools/wave_check.py, profiles/r04_wavefront.txt): fp32 at every size measured
    // (2 frames x 256 streams: 0.19 against 0.23 ms; 32 x 256: 1.13 against 2.52; 32 x 4 096: 11.4 against 13.5); bf16 up to 768 streams
    // (32 frames x 512 streams: 0.49 against 0.68 ms; 768: 0.66 against 0.73; 1 024: equal at best -- beyond, the chunked kernels'
    // resident weights win -- except in calls of 2-4 frames)
    const bool wave_wins = prec_ == kBf16 ? (mtb <= 48 || (mtb <= 64 && T <= 4)) : mtb <= 256;
    const bool wave = T > 1 && (dev_wave_mt_ >= 0 ? mtb <= dev_wave_mt_ : wave_wins) && !no_small_ && !debug_taps_ && (only < 0 || only == kClsGru) && wave_fits() &&
                      !resets;
    // One-frame bf16 calls whose m-tiles come in whole quads (from 60 m-tiles on): a GRU layer is ONE launch (kns_gruq.hip) -- input
    // GEMM, recurrent GEMM and gates fused over CU quads.  Same arithmetic as the two-kernel form, bit for bit
    // (tests/test_gpu_parity.py::test_alternative_kernels_give_identical_pcm).
    const bool quad = use_quad_ && !small && T == 1 && !resets;
    auto gru_quad = [&](const void *a0, int nb0, const void *a1, const void *wih, const float *bih, const void *whh,
                        const float *bhh, int layer, void *hseq, const StageDev *head = nullptr) {
        GruQuadArgs g;
        if (head) {  // the narrow head of the stage before, inside this launch (one-frame calls)
            g.yh = d_hseq_b_;
            g.yw = head->w_head;
            g.yb = head->b_head;
            g.yvalid = head->head_dim;
        }
        g.a0 = a0;
        g.a1 = a1;
        g.wih = wih;
        g.bih = bih;
        g.whh = whh;
        g.bhh = bhh;
        g.hstate_in = d_hstate_[hs_cur_] + (size_t) layer * mtb * kUnitTiles * 256;
        g.hstate_out = d_hstate_[hs_cur_ ^ 1] + (size_t) layer * mtb * kUnitTiles * 256;
        g.hseq = hseq;
        g.nb0 = nb0;
        g.mtiles = mtb;
        g.dbg = d_qdbg_;
        g.dbg_block = qdbg_block_;
        tick(kClsGru);
        if (only < 0 || only == kClsGru) launch_gru_quad(g, stream_);
        tock(kClsGru);
    };

    const bool small_steps = T > 1 && mtb <= steps_mt && prec_ != kBf16 && !no_small_ && !wave && !resets;
    last_head_launches_ = 0;
#ifdef KNS_DEV
    last_synth_launches_ = 0;
#endif
    last_route_ = resets ? kRouteChunkedResets : small ? kRouteSmall : wave ? kRouteWave : small_steps ? kRouteSmallSteps : quad ? kRouteQuad1 : kRouteChunked;
    // ---- mid-size batches: the layer pipeline over sub-chunks of frames (see the chunk loop below)
    const int pipe_chunk = dev_pipe_chunk_ > 0 ? dev_pipe_chunk_ : (T + 1) / 2;
    const int pipe_mt = dev_pipe_mt_ >= 0 ? dev_pipe_mt_ : 144;
    const int pipe_grid = dev_pipe_grid_ > 0 ? dev_pipe_grid_ : 128;
    const int pipe_streams = dev_pipe_streams_ > 0 && dev_pipe_streams_ <= kPipeStreams ? dev_pipe_streams_ : 2;
    const bool pipelined = !wave && !small && !small_steps && !quad && prec_ == kBf16 && mtb <= pipe_mt && T >= 32 && T >= 2 * pipe_chunk - 1 && !profiling_ &&
                           !debug_taps_ && only < 0 && !resets && pipe_ready();
    int nchunks = 1;
    if (pipelined) {
        nchunks = (T + pipe_chunk - 1) / pipe_chunk;
        if (T - (nchunks - 1) * pipe_chunk < pipe_chunk / 2 && nchunks > 2) --nchunks;  // (a short tail joins the last chunk)
    }
    // ... whose analysis and synthesis are cut into the same slices of frames when the spectrum is rebuilt from the PCM and the front-end
    // is folded (no launch between analysis and the first stage): slice c's analysis then runs beside slice c - 1's layers and slice
    // c's synthesis beside slice c + 1's -- 96 of a 1 024-stream call's 1 157 us were the two STFT launches alone at either end
    // (measured, tools/pipe_sweep.py: +1.3 % at 1 024 and 1 536 streams x 64 frames, nothing at 800, -0.3 % at 2 048; at 32 frames per call
    // -1 ... -1.5 % from 1 024 streams on -- the slices' launches then cost what their overlap gives: long calls of up to 112 m-tiles only)
    const bool stft_sliced = pipelined && fold_ && recompute && !an.write_spec && taps_ == 1 && !dev_pipe_whole_stft_ &&
                             (dev_pipe_chunk_ > 0 || (T >= 48 && mtb <= 112));
    auto analysis_slice = [&](int t0c, int Tc, bool first, bool last, hipStream_t st) {
        AnalysisArgs a = an;
        a.pcm = d_pcm + (size_t) t0c * kFrame;
        a.feat = feat_now + (size_t) t0c * feat_frame_bytes_;
        a.T = Tc;
        a.pitch = T;
        a.prev_in_pcm = first ? 0 : 1;
        a.write_hist = last ? 1 : 0;
        int seg = Tc;
        while (seg > 1 && (Bpad_ / 16) * ((Tc + seg - 1) / seg) < 1024) seg = (seg + 1) / 2;
        a.seg = dev_analysis_seg_ > 0 ? (dev_analysis_seg_ < Tc ? dev_analysis_seg_ : Tc) : seg;
#ifdef KNS_DEV
        last_analysis_seg_ = a.seg;
#endif
        launch_analysis(a, st);
    };
    if (!stft_sliced) {
        tick(kClsAnalysis);
#ifdef KNS_DEV
        last_analysis_seg_ = an.seg;
#endif
        if (only < 0 || only == kClsAnalysis) launch_analysis(an, stream_);
        tock(kClsAnalysis);
    }
    if (!in_place) hist_cur_ ^= 1;
    // front-end: e = features . W_in + b_in
    // (bf16 with a one-frame front-end: folded into the stage-input GEMMs, which read the features themselves -- no launch, no `e`)
    if (!fold_)
        gemm(kClsGemmHead, nullptr, 0, roll_in_analysis ? d_fhist_ : d_feat_, nbf_, w_in_, b_in_, d_e_, nbh_ * pi_.npb, kHidden, kOutAPlain,
             taps_);
    const void *stage_in = fold_ ? (const void *) feat_now : (const void *) d_e_;  // the e part of every stage's layer-A input
    if (taps_ > 1 && !roll_in_analysis)  // the last taps - 1 frames of [context | call] are the next call's context
        (void) hipMemcpyAsync(fhist_last, (char *) d_feat_ + (size_t) T * feat_frame_bytes_, (size_t) (taps_ - 1) * feat_frame_bytes_,
                              hipMemcpyDeviceToDevice, stream_);
    // One-frame calls through the quad kernel: the narrow head of stage s (271 -> 1, 5, 40) is computed inside stage s + 1's first
    // layer launch instead of in a launch of its own (kns_gruq.hip, kHead): 15 launches per frame step become 12.
    // ... and the mask head in the synthesis launch (bf16, stored spectrum -- what a one-frame call uses; kns_stft.hip, kMaskIn)
    const bool mask_in_synthesis = T == 1 && prec_ == kBf16 && fuse_front_ && !debug_taps_ && !recompute &&
                                   sd_[kStages - 1].head_tiles == kMaskTiles && !resets;
    mask_valid_ = !mask_in_synthesis;
    bool head_in_next = false;  // stage s - 1's head has been left to this stage's first layer
    bool head_in_recurrent = false;  // this stage's head was computed by its layer-B recurrent launch
    if (wave) {
        run_wave(T, mtb);
        if (!mask_in_synthesis)
            gemm(kClsGemmHead, nullptr, 0, d_hseq_b_, nbh_, sd_[kStages - 1].w_head, sd_[kStages - 1].b_head, d_mask_,
                 sd_[kStages - 1].head_tiles, kBins, kOutMask);
    }
    // Mid-size batches (round 6): with fewer than ~160 m-tiles the weight-resident recurrent launches occupy as many CUs and take the
    // same ~150 us per 64 frames as with 256 -- at 1 024 streams eight of them are 1.23 of the call's 1.37 ms on a quarter of the chip.
    // The layers of a call depend on each other frame by frame only, so the call is cut into sub-chunks of frames and the (layer, chunk)
    // grid runs as a wavefront over two streams: chunk c's 18 launches in order on stream c mod S, its recurrent launch of layer l
    // behind chunk c - 1's (an event per (chunk, layer)); up to S recurrent launches of different layers then share the chip.  Same
    // kernels on slices of the same buffers: the same bits (chunking is invisible).  Hidden state: chunk c reads ping-pong buffer
    // (hs_cur_ + c) & 1 and writes the other one.
    // Measured (tools/pipe_sweep.py, profiles/r06_pipe_sweep.txt): TWO sub-chunks on two streams is the best form at every size -- 64 frames x
    // 1 024 streams 1.34 -> 1.06 ms, x 2 048 streams 1.68 -> 1.48 ms; three chunks equal it, four and more lose (a launch of 8-16 frames is
    // mostly prologue, and every cross-stream event costs microseconds) -- and it stops paying at 160 m-tiles.
    // synthesis of frames [t0c, t0c + Tc) of the call (the whole call unless the STFT stages are sliced): slice number `ci` reads the
    // overlap-add tail from ping-pong buffer (tail_cur_ + ci) & 1 and leaves it in the other one
    auto synthesis_slice = [&](int t0c, int Tc, int ci, hipStream_t st) {
        SynthesisArgs sy;
        sy.spec = d_spec_;
        sy.mask = (const float *) ((const char *) d_mask_ + (size_t) t0c * mtb * kMaskTiles * 256 * (prec_ == kBf16 ? 2 : 4));
        sy.window = d_window_;
        sy.twiddle = d_twiddle_;
        const int tc = (tail_cur_ + ci) & 1;
        sy.tail_in = d_tail_[tc];
        sy.tail_out = d_tail_[in_place ? tc : tc ^ 1];
        const int seg_env = dev_synth_seg_;
        // two segments per stream tile (512 workgroups at B = 4096) measured best: fewer, longer segments amortise the
        // one replayed frame; a single segment leaves half the chip without a second workgroup to overlap with
        // ... and with few stream tiles the segments shrink (down to one frame) until there are about two workgroups per CU
        int seg_auto = Tc <= 4 ? Tc : ((Tc + 1) / 2 > 4 ? (Tc + 1) / 2 : 4);
        while (seg_auto > 1 && mtb * ((Tc + seg_auto - 1) / seg_auto) < 512) seg_auto = (seg_auto + 1) / 2;  // (few streams: down to one frame + its replay)
        const int seg = seg_env > 0 ? seg_env : seg_auto;
        sy.seg = Tc <= seg ? Tc : seg;
        sy.out = d_out + (size_t) t0c * kFrame;
        sy.pcm = d_pcm + (size_t) t0c * kFrame;
        sy.hist_in = hist_before;
        sy.recompute = recompute;
        sy.mask_fp16 = prec_ == kBf16;
        if (mask_in_synthesis) {
            sy.mask_h = d_hseq_b_;
            sy.mask_w = sd_[kStages - 1].w_head;
            sy.mask_b = sd_[kStages - 1].b_head;
        }
        sy.B = B_;
        sy.Bpad = Bpad_;
        sy.T = Tc;
        sy.pitch = T;
        sy.prev_in_pcm = t0c > 0 ? 1 : 0;
        sy.resets = rs;
        sy.rs_pitch = rs_pitch;
        sy.rs_t0 = rs_t0 + t0c;
        const CallSetup &cs = *slice.call;  // (what the call has prepared: read here and nowhere else below)
        sy.min_gain = cs.min_gain;
        sy.link = cs.link;
        sy.profile = cs.profile;
        if (cs.comfort_set) sy.comfort_amp = cs.comfort_amp, sy.comfort_set = cs.comfort_set, sy.comfort_n = d_cf_n_ + t0c;  // (like `report`: rows T frames apart)
        sy.report = slice.d_report ? slice.d_report + (size_t) t0c * 4 : nullptr;  // (like `out`: the slice's first frame, rows T frames apart)
#ifdef KNS_DEV
        last_synth_seg_ = sy.seg;
        ++last_synth_launches_;
#endif
        launch_synthesis(sy, st);
    };
    if (pipelined) (void) hipEventRecord(pipe_fork_, stream_);
    for (int c = 0; c < nchunks && !wave; ++c) {
      if (pipelined) {
          c_t0 = c * pipe_chunk;
          c_T = c == nchunks - 1 ? T - c_t0 : pipe_chunk;
          c_hs = (hs_cur_ + c) & 1;
          c_stream = pipe_stream_[c % pipe_streams];
          c_grid = pipe_grid;
          if (c < pipe_streams) (void) hipStreamWaitEvent(c_stream, pipe_fork_, 0);
          if (stft_sliced) analysis_slice(c_t0, c_T, c == 0, c == nchunks - 1, c_stream);
      }
      auto gru_dep = [&](const void *whh, const float *bhh, int layer, void *hseq, const StageDev *head = nullptr) {
          if (pipelined && c > 0) (void) hipStreamWaitEvent(c_stream, pipe_ev_[(c - 1) % kPipeRing][layer], 0);
          gru(whh, bhh, layer, hseq, head);
          if (pipelined && c + 1 < nchunks) (void) hipEventRecord(pipe_ev_[c % kPipeRing][layer], c_stream);
      };
      for (int s = 0; s < kStages; ++s) {
        const StageDev &d = sd_[s];
        head_in_recurrent = false;
        // (d.ypad: the previous head's few values sit in the padding of the features' last k-block -- no y part of its own)
        const void *yprev = s && !d.ypad ? d_y_[s - 1] : nullptr;
        const int nby = s && !d.ypad ? nby_[s - 1] : 0;
        if (small) {
            gru_small(yprev, nby, stage_in, d.w_ih_a, d.b_ih_a, d.w_hh_a, d.b_hh_a, 2 * s, d_hseq_a_, 0, head_in_next ? &sd_[s - 1] : nullptr);
            gru_small(nullptr, 0, d_hseq_a_, d.w_ih_b, d.b_ih_b, d.w_hh_b, d.b_hh_b, 2 * s + 1, d_hseq_b_);
        } else if (small_steps) {
            for (int t = 0; t < T; ++t) gru_small(yprev, nby, stage_in, d.w_ih_a, d.b_ih_a, d.w_hh_a, d.b_hh_a, 2 * s, d_hseq_a_, t);
            for (int t = 0; t < T; ++t)
                gru_small(nullptr, 0, d_hseq_a_, d.w_ih_b, d.b_ih_b, d.w_hh_b, d.b_hh_b, 2 * s + 1, d_hseq_b_, t);
        } else {
            if (quad && nby <= quad_nb0_max_) {
                gru_quad(yprev, nby, stage_in, d.w_ih_a, d.b_ih_a, d.w_hh_a, d.b_hh_a, 2 * s, d_hseq_a_, head_in_next ? &sd_[s - 1] : nullptr);
            } else {
                gemm(kClsGemmIn, yprev, nby, stage_in, nbh_, d.w_ih_a, d.b_ih_a, d_gi_, kGateTiles, 3 * kHidden, kOutGi);
                gru_dep(d.w_hh_a, d.b_hh_a, 2 * s, d_hseq_a_);
            }
            if (quad) {
                gru_quad(nullptr, 0, d_hseq_a_, d.w_ih_b, d.b_ih_b, d.w_hh_b, d.b_hh_b, 2 * s + 1, d_hseq_b_);
            } else {
                // multi-frame calls: a narrow head whose values go into the features' padding (stages 0 and 1) is computed by layer
                // B's recurrent kernel itself, step by step, while the hidden vectors are in LDS: two head launches and two passes
                // over a hidden sequence (2 x 151 MB at the bench shape) less -- and, the head GEMM below being that sequence's only
                // reader (the next stage's layer B overwrites d_hseq_b_, the last stage never carries its head), no sequence at all
                head_in_recurrent = T > 1 && s < kStages - 1 && sd_[s + 1].ypad && d.head_tiles == pi_.npb && fuse_head_ && !debug_taps_ &&
                                    !(dev_variant_ & kDevGruStream);
                gemm(kClsGemmIn, nullptr, 0, d_hseq_a_, nbh_, d.w_ih_b, d.b_ih_b, d_gi_, kGateTiles, 3 * kHidden, kOutGi);
                gru_dep(d.w_hh_b, d.b_hh_b, 2 * s + 1, d_hseq_b_, head_in_recurrent ? &d : nullptr);
            }
        }
        head_in_next = s < kStages - 1 && T == 1 && fuse_head_ && nby_[s] >= 1 && d.head_tiles == pi_.npb * nby_[s] && !debug_taps_ &&
                       (small || (quad && nby_[s] <= quad_nb0_max_));
        if (head_in_next || head_in_recurrent)
            ;
        else if (s < kStages - 1 && sd_[s + 1].ypad)  // into columns 257 ... of the features (k = 1 ... of their block 8)
            gemm(kClsGemmHead, nullptr, 0, d_hseq_b_, nbh_, d.w_head, d.b_head, feat_now, d.head_tiles, d.head_dim, kOutASigmoid, 1,
                 /*pad_nb=*/nbf_, /*pad_blk=*/kBins / pi_.kb, /*pad_kk0=*/kBins % pi_.kb);
        else if (s < kStages - 1)
            gemm(kClsGemmHead, nullptr, 0, d_hseq_b_, nbh_, d.w_head, d.b_head, d_y_[s], d.head_tiles, d.head_dim,
                 kOutASigmoid);
        else if (!mask_in_synthesis)
            gemm(kClsGemmHead, nullptr, 0, d_hseq_b_, nbh_, d.w_head, d.b_head, d_mask_, d.head_tiles, kBins, kOutMask);
    }
      if (stft_sliced) {  // this slice's synthesis, behind the previous slice's (the overlap-add tail goes from one to the next)
          if (c > 0) (void) hipStreamWaitEvent(c_stream, pipe_syn_[(c - 1) % kPipeRing], 0);
          synthesis_slice(c_t0, c_T, c, c_stream);
          if (c + 1 < nchunks) (void) hipEventRecord(pipe_syn_[c % kPipeRing], c_stream);
      }
      if (pipelined && (c >= nchunks - pipe_streams)) {  // the last chunk of each stream: the handle's stream continues behind it
          (void) hipEventRecord(pipe_join_[c % pipe_streams], c_stream);
          (void) hipStreamWaitEvent(stream_, pipe_join_[c % pipe_streams], 0);
      }
    }
    c_t0 = 0, c_T = T, c_hs = hs_cur_, c_stream = stream_, c_grid = 0;

    if (!stft_sliced) {
        tick(kClsSynthesis);
        if (only < 0 || only == kClsSynthesis) synthesis_slice(0, T, 0, stream_);
        tock(kClsSynthesis);
    }
    hs_cur_ = small_steps || wave ? (hs_cur_ + T) & 1 : pipelined ? (hs_cur_ + nchunks) & 1 : hs_cur_ ^ 1;
    if (pipelined) last_route_ = kRoutePipelined;
    if (!in_place) tail_cur_ = stft_sliced ? (tail_cur_ + nchunks) & 1 : tail_cur_ ^ 1;

    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = std::string("HIP launch error: ") + hipGetErrorString(e);
        return false;
    }
    return true;
}

static std::mutex g_capture_mutex;

enum PointerKind { kPtrPageable = 0, kPtrPinned = 1, kPtrDevice = 2 };

static PointerKind pointer_kind(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void) hipGetLastError();
        return kPtrPageable;
    }
    if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) return kPtrDevice;
    return attr.type == hipMemoryTypeHost ? kPtrPinned : kPtrPageable;
}

// rows x width bytes between pitched host buffers; large copies are split over a few threads (one core moves ~10 GB/s,
// which is a tenth of what the GPU consumes)
static void host_copy_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows) {
    auto span = [=](size_t r0, size_t r1) {
        if (dpitch == width && spitch == width) {
            memcpy((char *) dst + r0 * width, (const char *) src + r0 * width, (r1 - r0) * width);
            return;
        }
        for (size_t r = r0; r < r1; ++r) memcpy((char *) dst + r * dpitch, (const char *) src + r * spitch, width);
    };
    const size_t bytes = width * rows;
    unsigned hw = std::thread::hardware_concurrency();
    size_t nthreads = bytes >= ((size_t) 4 << 20) ? bytes >> 21 : 1;  // one thread per 2 MiB ...
    if (nthreads > 8) nthreads = 8;                                  // ... up to 8
    if (hw && nthreads > hw) nthreads = hw;
    if (nthreads > rows) nthreads = rows ? rows : 1;
    if (nthreads <= 1) {
        span(0, rows);
        return;
    }
    std::vector<std::thread> pool;
    for (size_t i = 1; i < nthreads; ++i) pool.emplace_back(span, rows * i / nthreads, rows * (i + 1) / nthreads);
    span(0, rows / nthreads);
    for (std::thread &t : pool) t.join();
}

// Host-pointer call in sub-chunks of host_chunk_ frames: H2D of chunk c+1, the kernels of chunk c and D2H of chunk c-1 run
// on three streams.  Pinned user buffers (hipHostMalloc / hipHostRegister / pv_koala_batch_host_alloc) are read and written
// by the copy engines directly (strided 2D copies); pageable ones go through the engine's pinned staging slots.
// The sub-chunk lengths of a synchronous host call of T frames.  What the caller waits for is
//   copy-in(first chunk) + sum of the chunks' kernel times + copy-out(last chunk),
// and a chunk's kernels cost ~0.17 ms of weight-resident prologues whatever its length (16 launches): short chunks at the two ENDS
// (little exposed copy time), long ones in the middle (few prologues) -- for 64 frames 4 8 12 16 12 8 4 instead of 4 x 16: 57.8 -> 61.6 M
// frames/s with page-locked buffers (profiles/r05_host_sched.txt; a model with the measured copy rate and K(T) had said 61.5).  No chunk
// exceeds host_chunk_ (a staging slot).
std::vector<int> Engine::host_schedule(int T) const {
    std::vector<int> sched;
    if (!dev_host_sched_.empty()) {  // developer override: the given lengths, repeated / truncated to T
        int left = T;
        for (size_t i = 0; left > 0; ++i) {
            const int c = std::min(left, std::max(1, std::min(host_chunk_, dev_host_sched_[i % dev_host_sched_.size()])));
            sched.push_back(c);
            left -= c;
        }
        return sched;
    }
    // a ramp of P/4, P/2, 3P/4 frames at either end (as many of its steps as the call has room for), chunks of at most P between them
    const int P = host_chunk_;
    int ramp[3] = {std::max(1, P / 4), std::max(1, P / 2), std::max(1, (3 * P) / 4)}, steps = 3;
    while (steps > 0 && 2 * (ramp[0] + (steps > 1 ? ramp[1] : 0) + (steps > 2 ? ramp[2] : 0)) + P > T) --steps;
    int ends = 0;
    for (int i = 0; i < steps; ++i) ends += ramp[i];
    const int mid = T - 2 * ends, n = (mid + P - 1) / P;
    for (int i = 0; i < steps; ++i) sched.push_back(ramp[i]);
    for (int i = 0; i < n; ++i) sched.push_back(mid / n + (i < mid % n ? 1 : 0));
    for (int i = steps - 1; i >= 0; --i) sched.push_back(ramp[i]);
    return sched;
}

bool Engine::process_host_pipelined(const Call &call, bool pinned, CallSetup *setup, std::string *err) {
    const int T = call.T;
    const int16_t *pcm = call.pcm;
    int16_t *out = call.out;
    const std::vector<int> sched = host_schedule(T);
    const int n = (int) sched.size();
    std::vector<int> first(n + 1, 0);  // first frame of chunk c
    for (int c = 0; c < n; ++c) first[c + 1] = first[c] + sched[c];
    const size_t row_user = (size_t) T * kFrame * 2;           // pitch of the caller's [B][T * 256] matrices
    const size_t slot = (size_t) B_ * host_chunk_ * kFrame;    // int16 elements per staging slot (the longest chunk fits)
    bool ok = true;
    auto check = [&](hipError_t e) { ok = ok && e == hipSuccess; };
    // (the frame report, when asked for, travels beside the samples: staged per sub-chunk as [B][tc][4] in slot s of d_report_ / h_report_)
    float *report = call.report;
    const size_t rslot = (size_t) B_ * host_chunk_ * 4, rrow_user = (size_t) T * 16;
    auto drain_to_user = [&](int c) {  // chunk c's output: staging slot -> caller (pageable path)
        const int s = c & 1, tc = sched[c];
        check(hipEventSynchronize(ev_out_[s]));
        host_copy_2d((char *) out + (size_t) first[c] * kFrame * 2, row_user, h_out_ + s * slot, (size_t) tc * kFrame * 2,
                     (size_t) tc * kFrame * 2, B_);
        if (report) host_copy_2d((char *) report + (size_t) first[c] * 16, rrow_user, h_report_ + s * rslot, (size_t) tc * 16, (size_t) tc * 16, B_);
    };
    for (int c = 0; c < n && ok; ++c) {
        const int s = c & 1, tc = sched[c];
        const size_t width = (size_t) tc * kFrame * 2;
        const char *src = (const char *) pcm + (size_t) first[c] * kFrame * 2;
        // ---- copy-in (slot s was last read by the kernels of chunk c - 2)
        if (c >= 2) check(hipStreamWaitEvent(copy_in_, ev_done_[s], 0));
        if (pinned) {
            check(hipMemcpy2DAsync(d_in_ + s * slot, width, src, row_user, width, B_, hipMemcpyHostToDevice, copy_in_));
        } else {
            if (c >= 2) check(hipEventSynchronize(ev_in_[s]));  // the H2D of chunk c - 2 has left the staging slot
            host_copy_2d(h_in_ + s * slot, width, src, row_user, width, B_);
            check(hipMemcpyAsync(d_in_ + s * slot, h_in_ + s * slot, width * B_, hipMemcpyHostToDevice, copy_in_));
        }
        check(hipEventRecord(ev_in_[s], copy_in_));
        // ---- kernels (d_out_ slot s was last drained by the D2H of chunk c - 2)
        check(hipStreamWaitEvent(stream_, ev_in_[s], 0));
        if (c >= 2) check(hipStreamWaitEvent(stream_, ev_out_[s], 0));
        if (ok && !run_device({first[c], tc, d_in_ + s * slot, d_out_ + s * slot, true, report ? d_report_ + s * rslot : nullptr, setup}, err)) {
            // copies of earlier sub-chunks may still be writing into the caller's buffers: let them finish first
            (void) hipStreamSynchronize(copy_in_);
            (void) hipStreamSynchronize(copy_out_);
            (void) hipStreamSynchronize(stream_);
            return false;
        }
        check(hipEventRecord(ev_done_[s], stream_));
        // ---- copy-out
        check(hipStreamWaitEvent(copy_out_, ev_done_[s], 0));
        if (pinned) {
            check(hipMemcpy2DAsync((char *) out + (size_t) first[c] * kFrame * 2, row_user, d_out_ + s * slot, width, width, B_,
                                   hipMemcpyDeviceToHost, copy_out_));
            if (report)
                check(hipMemcpy2DAsync((char *) report + (size_t) first[c] * 16, rrow_user, d_report_ + s * rslot, (size_t) tc * 16, (size_t) tc * 16,
                                       B_, hipMemcpyDeviceToHost, copy_out_));
        } else {
            if (c >= 2) drain_to_user(c - 2);  // frees staging slot s
            check(hipMemcpyAsync(h_out_ + s * slot, d_out_ + s * slot, width * B_, hipMemcpyDeviceToHost, copy_out_));
            if (report) check(hipMemcpyAsync(h_report_ + s * rslot, d_report_ + s * rslot, (size_t) tc * 16 * B_, hipMemcpyDeviceToHost, copy_out_));
        }
        check(hipEventRecord(ev_out_[s], copy_out_));
    }
    if (ok && !pinned) {
        if (n >= 2) drain_to_user(n - 2);
        drain_to_user(n - 1);
    }
    if (ok && pinned) {
        check(hipEventSynchronize(ev_out_[(n - 1) & 1]));
        if (n >= 2) check(hipEventSynchronize(ev_out_[(n - 2) & 1]));
    }
    if (ok) check(hipStreamSynchronize(stream_));
    if (!ok) {
        *err = hip_last_error();
        (void) hipDeviceSynchronize();
        return false;
    }
    return true;
}

void Engine::set_stream(hipStream_t s) {
    hipStream_t next = s ? s : own_stream_;
    if (next == stream_) return;
    (void) hipSetDevice(device_);
    std::string ignored;
    (void) drain_async(&ignored);
    if (hipStreamSynchronize(stream_) != hipSuccess) (void) hipGetLastError();
    stream_ = next;
}

bool Engine::drain_async(std::string *err) {
    bool ok = true;
    for (int i = 0; i < 4; ++i) {
        if (!async_busy_[i]) continue;
        if (hipEventSynchronize(aev_out_[i]) != hipSuccess) ok = false;
        async_busy_[i] = false;
    }
    if (!ok) {
        *err = hip_last_error();
        (void) hipDeviceSynchronize();
    }
    return ok;
}

bool Engine::async_wait(int max_in_flight, std::string *err) {
    if (max_in_flight <= 0) return drain_async(err);
    for (int j = 3; j > max_in_flight; --j) {  // the calls async_n_ - 3 ... async_n_ - max_in_flight - 1, oldest first
        if ((unsigned) j > async_n_) continue;
        const int ring = (int) ((async_n_ - (unsigned) j) & 3u);
        if (!async_busy_[ring]) continue;
        if (hipEventSynchronize(aev_out_[ring]) != hipSuccess) {
            *err = hip_last_error();
            return false;
        }
        async_busy_[ring] = false;
    }
    return true;
}

// One asynchronous host call = H2D on copy_in_, the kernels on the handle's stream, D2H on copy_out_, chained by events.  Up to
// THREE calls are in flight: with two, a caller alternating between two buffer pairs cannot issue call n + 2 before call n's copy-out has
// finished, which puts a slot's copy-in, kernels and copy-out in series (measured: 4.03 ms per 4096 x 64 frames = (2.8 + 2.6 + 2.8) / 2);
// with three, the link works in both directions under the kernels (~48 GB/s each way at once, profiles/r05_pcie_probe.txt).  Device
// staging alternates between two slots: the input half of slot s is free once the kernels of call n - 2 have read it, the output half
// once call n - 2's copy-out has -- both waited for on the device, by the stream that needs it.  A synchronous call of that size cannot
// hide its first copy-in and last copy-out and has to cut its kernels into short, less efficient sub-chunks (process_host_pipelined).
Status Engine::process_host_async(const Call &c, std::string *err) {
    if (refuse_stages(c.opt, " is not available yet on the asynchronous entry points.", err)) return Status::kBadArgument;
    if (c.opt.channel_link) {  // (its slices carry no link; the owner refuses the asynchronous calls on a handle with channels anyway)
        *err = "linked channels are not available in asynchronous calls.";
        return Status::kBadArgument;
    }
    if (fmt_ != kFmtS16) {
        *err = "asynchronous calls are not available on a handle whose sample format is not S16.";
        return Status::kBadArgument;
    }
    if (rate_ != kRate16k) {
        *err = "asynchronous calls are not available on a handle whose sample rate is not 16000.";
        return Status::kBadArgument;
    }
    if (c.hold) {
        *err = "asynchronous host calls take no held streams.";
        return Status::kBadArgument;
    }
    const int T = c.T;
    const int16_t *pcm = c.pcm;
    int16_t *out = c.out;
    (void) hipSetDevice(device_);
    if (pointer_kind(pcm) != kPtrPinned || pointer_kind(out) != kPtrPinned) {
        *err = "asynchronous host calls need page-locked `pcm` and `enhanced` (pv_koala_batch_host_alloc, hipHostMalloc or hipHostRegister).";
        return Status::kRuntime;
    }
    if (c.report && pointer_kind(c.report) != kPtrPinned) {
        *err = "asynchronous host calls need a page-locked `report` (pv_koala_batch_host_alloc, hipHostMalloc or hipHostRegister).";
        return Status::kRuntime;
    }
    const size_t bytes = (size_t) B_ * T * kFrame * 2;
    {
        const char *pa = (const char *) pcm, *pb = (const char *) out;
        if (pa != pb && pa < pb + bytes && pb < pa + bytes) {
            *err = "`pcm` and `enhanced` overlap partially.";
            return Status::kRuntime;
        }
    }
    if (c.report && !report_ready(true, err)) return Status::kRuntime;
    if (!async_ready_) {  // set only once EVERY event and both buffers exist: a partial failure is retried by the next call
        bool ok = true;
        for (int i = 0; i < 4 && ok; ++i)
            if (!aev_out_[i]) ok = hipEventCreateWithFlags(&aev_out_[i], hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i) {
            if (!aev_in_[i]) ok = hipEventCreateWithFlags(&aev_in_[i], hipEventDisableTiming) == hipSuccess;
            if (ok && !aev_done_[i]) ok = hipEventCreateWithFlags(&aev_done_[i], hipEventDisableTiming) == hipSuccess;
        }
        if (ok && !d_in2_) d_in2_ = (int16_t *) dalloc((size_t) B_ * Tmax_ * kFrame * 2, false);
        if (ok && !d_out2_) d_out2_ = (int16_t *) dalloc((size_t) B_ * Tmax_ * kFrame * 2, false);
        ok = ok && d_in2_ && d_out2_;
        if (!ok) {
            (void) hipGetLastError();
            *err = "Failed to allocate the second staging slot of asynchronous host calls.";
            return Status::kRuntime;
        }
        async_ready_ = true;
    }
    const unsigned n = async_n_;
    const int s = (int) (n & 1u), ring = (int) (n & 3u), ring3 = (int) ((n - 3u) & 3u), ring2 = (int) ((n - 2u) & 3u);
    if (n >= 3 && async_busy_[ring3]) {  // the window: the call three back has completed before this one is accepted
        if (hipEventSynchronize(aev_out_[ring3]) != hipSuccess) {
            *err = hip_last_error();
            return Status::kRuntime;
        }
        async_busy_[ring3] = false;
    }
    CallSetup setup;  // (this call keeps the mask, the gains and the profile it was issued under: the caller may change them now)
    if (!begin_call(c, false, &setup, err)) return Status::kRuntime;
    int16_t *din = s ? d_in2_ : d_in_, *dout = s ? d_out2_ : d_out_;
    float *drep = c.report ? (s ? d_report2_ : d_report_) : nullptr;  // (part of the call's staging slot: free when its samples' slot is)
    bool ok = true;
    if (n >= 2) ok = hipStreamWaitEvent(copy_in_, aev_done_[s], 0) == hipSuccess;  // the kernels of call n - 2 have read this slot's input
    ok = ok && hipMemcpyAsync(din, pcm, bytes, hipMemcpyHostToDevice, copy_in_) == hipSuccess;
    ok = ok && hipEventRecord(aev_in_[s], copy_in_) == hipSuccess;
    ok = ok && hipStreamWaitEvent(stream_, aev_in_[s], 0) == hipSuccess;
    if (n >= 2) ok = ok && hipStreamWaitEvent(stream_, aev_out_[ring2], 0) == hipSuccess;  // ... and its copy-out this slot's output
    if (!ok) {
        *err = hip_last_error();
        (void) hipDeviceSynchronize();  // (a copy-in may have been enqueued: nothing of this call stays in flight)
        return Status::kRuntime;
    }
    if (!run_device({0, T, din, dout, true, drep, &setup}, err)) {
        (void) hipDeviceSynchronize();
        return Status::kRuntime;
    }
    ok = hipEventRecord(aev_done_[s], stream_) == hipSuccess;
    ok = ok && hipStreamWaitEvent(copy_out_, aev_done_[s], 0) == hipSuccess;
    // (as a 2-D copy of B_ rows: the runtime hands those to the copy engines; a plain hipMemcpyAsync into page-locked memory went
    // through its copy KERNEL, which took compute units from the engine's own kernels -- profiles/r05_host_async_trace.txt)
    ok = ok && hipMemcpy2DAsync(out, (size_t) T * kFrame * 2, dout, (size_t) T * kFrame * 2, (size_t) T * kFrame * 2, B_, hipMemcpyDeviceToHost,
                                copy_out_) == hipSuccess;
    if (drep)  // (in front of the call's completion event: the report is valid when the call has completed)
        ok = ok && hipMemcpy2DAsync(c.report, (size_t) T * 16, drep, (size_t) T * 16, (size_t) T * 16, B_, hipMemcpyDeviceToHost, copy_out_) == hipSuccess;
    ok = ok && hipEventRecord(aev_out_[ring], copy_out_) == hipSuccess;
    if (!ok) {
        *err = hip_last_error();
        (void) hipDeviceSynchronize();
        return Status::kRuntime;
    }
    async_busy_[ring] = true;
    ++async_n_;
    return Status::kOk;
}

bool Engine::run_call(const Call &c, std::string *err) {
    const int T = c.T;
    const int16_t *pcm = c.pcm;
    int16_t *out = c.out;
    (void) hipSetDevice(device_);
    if (async_n_ && !drain_async(err)) return false;
    const size_t bytes = (size_t) B_ * T * kFrame * 2;
    // (the single-stream ABI takes host buffers by contract: no driver query per frame on the latency path)
    const PointerKind kin = c.host_contract ? kPtrPageable : pointer_kind(pcm), kout = c.host_contract ? kPtrPageable : pointer_kind(out);
    if ((kin == kPtrDevice) != (kout == kPtrDevice)) {
        *err = "`pcm` and `enhanced` must both be host or both be device memory.";
        return false;
    }
    float *report = c.report;
    if (report && !c.host_contract && (pointer_kind(report) == kPtrDevice) != (kout == kPtrDevice)) {
        *err = "`report` must be memory of the same kind as `enhanced`: host with host, device with device.";
        return false;
    }
    if (report && kin != kPtrDevice && !report_ready(false, err)) return false;
    const size_t rbytes = (size_t) B_ * T * 16;
    const bool pipelined = kin != kPtrDevice && T > host_chunk_ && bytes >= host_pipeline_min_bytes_;
    const char *pa = (const char *) pcm, *pb = (const char *) out;
    // partial overlap: chunk c's copy-out would land on input chunks not yet read.  EXACT aliasing (enhanced == pcm) is fine:
    // chunk c's output columns are chunk c's own input columns, which have been staged by then
    if (pipelined && pa != pb && pa < pb + bytes && pb < pa + bytes) {
        *err = "`pcm` and `enhanced` overlap: host-memory calls of this size are pipelined in sub-chunks and need disjoint buffers.";
        return false;
    }
    CallSetup setup;  // (this call's tables, on the handle's stream in front of everything below: nothing of it outlives the call)
    if (!begin_call(c, kin == kPtrDevice, &setup, err)) return false;
    if (kin == kPtrDevice) {
        const size_t n = (size_t) B_ * T * kFrame;
        const bool overlap = pcm < out + n && out < pcm + n;
        // (a levelling call reads its own report -- an output only, so asking for it into a buffer of the engine's changes no bit)
        float *rep = (setup.stages & kStageLevel) && !report ? d_lv_rep_ : report;
        // (comfort noise: the counter's launch in front of the call's kernels; the limiter's stands in the place of the leveller's second one)
        return (!(setup.stages & kStageComfort) || run_comfort(c, setup, err)) && run_device({0, T, pcm, out, !overlap, rep, &setup}, err) &&
               (!(setup.stages & (kStageLevel | kStageLimiter)) || run_level(c, rep, report != nullptr, setup, err));
    }
    if (pipelined) {
        // On a caller's stream the kernels of the sub-chunks still run on the handle's OWN stream, fenced behind whatever the caller
        // has enqueued (the call is synchronous, so everything the caller enqueues later is behind it anyway): the handle's three
        // streams were created together and sit on three different hardware queues, while a foreign stream may share its queue with
        // one of the copy streams -- measured: 40 instead of 62 M frames/s for page-locked buffers (profiles/r06_bench.json notes)
        hipStream_t user = stream_;
        if (user != own_stream_ && !profiling_) {
            if (!host_fork_ && hipEventCreateWithFlags(&host_fork_, hipEventDisableTiming) != hipSuccess) {
                (void) hipGetLastError();
                host_fork_ = nullptr;
            }
            if (host_fork_ && hipEventRecord(host_fork_, user) == hipSuccess && hipStreamWaitEvent(own_stream_, host_fork_, 0) == hipSuccess)
                stream_ = own_stream_;
        }
        const bool pinned = kin == kPtrPinned && kout == kPtrPinned && (!report || pointer_kind(report) == kPtrPinned);
        const bool done = process_host_pipelined(c, pinned, &setup, err);
        stream_ = user;
        return done;
    }
    memcpy(h_in_, pcm, bytes);
    if (T == 1 && use_graph_ && stream_ == own_stream_ && !profiling_ && !setup.link) {
        // frame-by-frame streaming: (copy-in,) the kernels of one frame (and copy-out) replayed as one hipGraph.  A handle that crosses
        // between "no limit" and "some limit", asking and not asking for the report, or a profile and none changes graphs; a change of a
        // table's values only re-uploads it, which begin_call has put on the stream in front of the replay
        const int hs = hs_cur_;
        const int parity = frame_graph_index(setup, report != nullptr);
        if (!frame_graph_[parity]) {
            hipGraph_t graph = nullptr;
            // (relaxed mode and one capture at a time in the process: other threads -- other handles being created, the
            // host application -- may touch the legacy stream meanwhile, which would invalidate a stricter capture)
            std::lock_guard<std::mutex> capture_lock(g_capture_mutex);
            bool ok = hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed) == hipSuccess;
            if (ok) {
                // small batches: the analysis kernel reads the frame from, and the synthesis kernel writes it to, the
                // pinned host staging buffers directly (device-visible memory): two copy nodes of ~4 us each less per frame
                const bool zero_copy = bytes <= 64 * 1024 && !no_zero_copy_;
                ok = zero_copy || hipMemcpyAsync(d_in_, h_in_, bytes, hipMemcpyHostToDevice, stream_) == hipSuccess;
                // (no reset table in the captured frame, whichever call happens to capture it: a one-frame call can restart a stream
                // at frame 0 only, and that is the reset kernel begin_resets has already put in front of the graph)
                Slice frame{0, 1, zero_copy ? h_in_ : d_in_, zero_copy ? h_out_ : d_out_, true, report ? (zero_copy ? h_report_ : d_report_) : nullptr, &setup};
                frame.without_reset_table = true;
                ok = ok && run_device(frame, err);
                ok = ok && (zero_copy || hipMemcpyAsync(h_out_, d_out_, bytes, hipMemcpyDeviceToHost, stream_) == hipSuccess);
                ok = ok && (zero_copy || !report || hipMemcpyAsync(h_report_, d_report_, rbytes, hipMemcpyDeviceToHost, stream_) == hipSuccess);
                // zero-copy frames end with the completion word (the output is already in host memory when that node runs)
                frame_graph_signals_[parity] = ok && zero_copy && spin_wait_ && h_frame_word_ && d_frame_count_;
                if (frame_graph_signals_[parity]) launch_frame_done(d_frame_count_, h_frame_word_, stream_);
                ok = (hipStreamEndCapture(stream_, &graph) == hipSuccess) && ok;
                ok = ok && hipGraphInstantiate(&frame_graph_[parity], graph, nullptr, nullptr, 0) == hipSuccess;
                if (graph) (void) hipGraphDestroy(graph);
            }
            hs_cur_ = hs;  // the capture only recorded the launches; run_device's bookkeeping is replayed below
            if (!ok) {
                // a failed capture must not leave the handle half-switched: nothing was executed, the ping-pong index is
                // back where it was, and this and every later frame take the plain copy / launch / copy path below
                (void) hipGetLastError();
                frame_graph_[parity] = nullptr;
                use_graph_ = false;
            }
        }
        if (use_graph_) {
            if (hipGraphLaunch(frame_graph_[parity], stream_) != hipSuccess) goto fail;
            hs_cur_ = hs ^ 1;
            if (frame_graph_signals_[parity]) {
                // Poll the frame's completion word (a frame takes 50-100 us: longer than the runtime's own active-wait window,
                // after which hipStreamSynchronize sleeps on an interrupt and wakes up whenever the host scheduler gets to it).
                // The first ~250 us -- two to five frame times -- in a tight loop, then yielding the core between polls (a host that
                // runs more handles than cores must not have its pollers starve each other); a frame that has not reported
                // after 20 ms is handed to hipStreamSynchronize, which also surfaces errors.
                const unsigned want = ++frame_seq_;
                const auto t0 = std::chrono::steady_clock::now();
                bool seen = false, yielding = false;
                for (unsigned spins = 0;; ++spins) {
                    if (__atomic_load_n(h_frame_word_, __ATOMIC_ACQUIRE) == want) {
                        seen = true;
                        break;
                    }
                    if (yielding) {
                        std::this_thread::yield();
                    } else {
#if defined(__x86_64__) || defined(__i386__)
                        __builtin_ia32_pause();
#elif defined(__aarch64__)
                        asm volatile("yield" ::: "memory");
#endif
                    }
                    if (yielding || (spins & 0xff) == 0xff) {
                        const auto dt = std::chrono::steady_clock::now() - t0;
                        if (dt > std::chrono::milliseconds(20)) break;
                        yielding = dt > std::chrono::microseconds(250);
                    }
                }
                if (!seen) {
                    if (hipStreamSynchronize(stream_) != hipSuccess) goto fail;
                    frame_seq_ = __atomic_load_n(h_frame_word_, __ATOMIC_ACQUIRE);  // (resynchronise the expectation)
                } else if ((want & 1023u) == 0) {
                    // (now and then: lets the runtime retire the launches it has been tracking; returns at once, the stream is idle)
                    if (hipStreamSynchronize(stream_) != hipSuccess) goto fail;
                }
            } else if (hipStreamSynchronize(stream_) != hipSuccess) {
                goto fail;
            }
            memcpy(out, h_out_, bytes);
            if (report) memcpy(report, h_report_, rbytes);  // (written by the synthesis kernel in front of the completion word)
            return true;
        }
    }
    if (hipMemcpyAsync(d_in_, h_in_, bytes, hipMemcpyHostToDevice, stream_) != hipSuccess) goto fail;
    if (!run_device({0, T, d_in_, d_out_, true, report ? d_report_ : nullptr, &setup}, err)) return false;
    if (hipMemcpyAsync(h_out_, d_out_, bytes, hipMemcpyDeviceToHost, stream_) != hipSuccess) goto fail;
    if (report && hipMemcpyAsync(h_report_, d_report_, rbytes, hipMemcpyDeviceToHost, stream_) != hipSuccess) goto fail;
    if (hipStreamSynchronize(stream_) != hipSuccess) goto fail;
    memcpy(out, h_out_, bytes);
    if (report) memcpy(report, h_report_, rbytes);
    return true;
fail:
    *err = hip_last_error();
    return false;
}

// ------------------------------------------------------------------------------------------------ handles that are not at 16 kHz

// High-band carry (Call::high_band): at the first such call the state's three ping-pong pairs and the engine's own report buffer; at that call and at
// a call whose epoch is not the last one seen -- the owner turned the feature on again -- the state is cleared on the handle's stream, so the
// high band is that of streams that begin with this call.
bool Engine::high_band_ready(const Call &c, std::string *err) {
    const int R = rs_stage_out(rate_).U;
    if (!d_hb_rep_) {
        for (int k = 0; k < 2; ++k) {
            if (!d_hb_x_[k]) d_hb_x_[k] = (int16_t *) dalloc((size_t) Bpad_ * hb_x_hist(R) * 2, false);
            if (!d_hb_y_[k]) d_hb_y_[k] = (int16_t *) dalloc((size_t) Bpad_ * kHbYHist * 2, false);
            if (!d_hb_s_[k]) d_hb_s_[k] = (float *) dalloc((size_t) Bpad_ * 2 * 4, false);
        }
        float *rep = d_hb_x_[0] && d_hb_x_[1] && d_hb_y_[0] && d_hb_y_[1] && d_hb_s_[0] && d_hb_s_[1] ? (float *) dalloc((size_t) B_ * Tmax_ * 16, false) : nullptr;
        if (!rep) {
            (void) hipGetLastError();
            *err = "Failed to allocate the buffers of the high-band carry.";
            return false;
        }
        d_hb_rep_ = rep;
        hb_epoch_ = c.high_band_epoch - 1;  // (cleared below, on the stream the call runs on)
    }
    if (hb_epoch_ != c.high_band_epoch) {
        launch_high_band_reset(d_hb_x_, d_hb_y_, d_hb_s_, R, nullptr, Bpad_, stream_);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            *err = hip_error(e);
            return false;
        }
        hb_epoch_ = c.high_band_epoch;
    }
    return true;
}

// A call of a handle that is not at 16 kHz (third extension): the in-stage kernel takes the caller's samples to 16 kHz
// (into d_in_), the call runs unchanged as a device-pointer call from d_in_ to d_out_ -- its resets, attenuation limit and frame report
// with it -- and the out-stage kernel takes the enhanced samples to the caller's rate.  Everything is enqueued on the handle's stream.
// Device pointers only, and no refusal of its own: host memory and every argument check are the entry's (process, run_packets).  The
// in-stage has read all of `pcm` before the out-stage writes `out`, so the two may overlap in any way.  The call's per-frame resets go to
// the device as they are (uint8 [B][T]): both stages read everything in front of a reset block as zero.  The rates differ in the stages'
// (U, D) and tables only.
bool Engine::run_call_rate(const Call &c, std::string *err) {
    const int T = c.T;
    (void) hipSetDevice(device_);
    bool any = false;
    for (size_t i = 0; c.resets && i < (size_t) B_ * T && !any; ++i) any = c.resets[i] != 0;
    const uint8_t *flags = nullptr;
    if (any) {
        if (!rsf_up_.ready(this, (size_t) B_ * Tmax_)) {
            *err = "Failed to allocate the buffers of per-frame stream resets.";
            return false;
        }
        int k;
        void *slot = rsf_up_.take(&k);
        if (!slot) goto fail;
        memcpy(slot, c.resets, (size_t) B_ * T);
        if (!rsf_up_.send(k, (size_t) B_ * T, stream_)) goto fail;
        flags = (const uint8_t *) rsf_up_.d;
    }
    if (c.high_band && !high_band_ready(c, err)) return false;
    {
        Call inner{T, d_in_, d_out_, c.resets};
        inner.opt = c.opt;
        inner.report = c.report;
        // (output stages: they work on the inner 16 kHz samples, between the call and the out-stage; `hold` rides along for their state
        // alone -- process_frames has put the held streams' records aside around this whole call)
        if (c.opt.level || c.opt.limiter || c.opt.comfort) inner.hold = c.hold;
        // High-band carry: the kernel behind the out-stage reads the call's masks from its report -- an output only, so asking for it into a
        // buffer of the engine's changes no bit -- the in-stage's rows, which the device-pointer call leaves in d_in_ as they are, and the
        // call's input, of which a copy is kept where the out-stage writes over it.
        const size_t n_io = (size_t) B_ * T * rs_frame_length(rate_);
        const int16_t *hb_x = c.pcm;
        if (c.high_band) {
            if (!inner.report) inner.report = d_hb_rep_;
            if (c.pcm < c.out + n_io && c.out < c.pcm + n_io) {
                if (!d_hb_in_) d_hb_in_ = (int16_t *) dalloc((size_t) B_ * Tmax_ * rs_frame_length(rate_) * 2, false);
                if (!d_hb_in_) {
                    (void) hipGetLastError();
                    *err = "Failed to allocate the buffers of the high-band carry.";
                    return false;
                }
                if (hipMemcpyAsync(d_hb_in_, c.pcm, n_io * 2, hipMemcpyDeviceToDevice, stream_) != hipSuccess) goto fail;
                hb_x = d_hb_in_;
            }
        }
        const RsStage si = rs_stage_in(rate_), so = rs_stage_out(rate_);
        ResampleArgs a;
        a.B = B_, a.T = T, a.resets = flags;
        a.q_frame = kFrame / si.U;  // (a group is U_in = D_out samples at 16 kHz)
        for (int k = 0; k < 2; ++k) {  // the in-stage, the call between the two, the out-stage
            a.U = k ? so.U : si.U, a.D = k ? so.D : si.D;
            a.in = k ? d_out_ : c.pcm, a.out = k ? c.out : d_in_;
            a.state = d_rs_state_[k][rs_cur_], a.state_next = d_rs_state_[k][rs_cur_ ^ 1];
            memcpy(a.taps, rs_taps_[k].data(), sizeof(a.taps));
            launch_resample(a, stream_);
            if (hipGetLastError() != hipSuccess) goto fail;
            if (k == 0 && !run_call(inner, err)) return false;
        }
        rs_cur_ ^= 1;
        if (c.high_band) {
            HighBandArgs h;
            h.x = hb_x, h.y = d_in_, h.out = c.out, h.report = inner.report;
            h.min_gain = c.opt.min_gain ? (const float *) mg_tab_.up.d : nullptr;  // (the inner call's begin_call has put the table on the stream)
            h.resets = flags;
            h.xs = d_hb_x_[hb_cur_], h.ys = d_hb_y_[hb_cur_], h.ss = d_hb_s_[hb_cur_];
            h.xs_next = d_hb_x_[hb_cur_ ^ 1], h.ys_next = d_hb_y_[hb_cur_ ^ 1], h.ss_next = d_hb_s_[hb_cur_ ^ 1];
            h.B = B_, h.T = T, h.R = so.U, h.link = c.opt.channel_link ? ch_ : 0;
            memcpy(h.taps, rs_taps_[1].data(), sizeof(h.taps));
            launch_high_band(h, stream_);
            if (hipGetLastError() != hipSuccess) goto fail;
            hb_cur_ ^= 1;
        }
    }
    return true;
fail:
    *err = hip_last_error();
    return false;
}

// ------------------------------------------------------------------------------------------------ output leveller

// The call's `hold` and reset flags as one row of T + 1 bytes per stream (run_call: in front of the call's first launch), only when one of
// them is set: the comfort counter's launch, the leveller's tracker and the limiter's launch read the same rows.
bool Engine::control_rows(const Call &c, const uint8_t **ctl, std::string *err) {
    const int T = c.T;
    bool any = false;
    for (int b = 0; c.hold && b < B_ && !any; ++b) any = c.hold[b] != 0;
    for (size_t i = 0; c.resets && i < (size_t) B_ * T && !any; ++i) any = c.resets[i] != 0;
    *ctl = nullptr;
    if (!any) return true;
    int k;
    uint8_t *rows = (uint8_t *) ctl_up_.take(&k);
    if (rows) {
        for (int b = 0; b < B_; ++b) {
            uint8_t *row = rows + (size_t) b * (T + 1);
            row[0] = c.hold && c.hold[b] ? 1 : 0;
            for (int t = 0; t < T; ++t) row[1 + t] = c.resets && c.resets[(size_t) b * T + t] ? 1 : 0;
        }
    }
    if (!rows || !ctl_up_.send(k, (size_t) B_ * (T + 1), stream_)) {
        *err = hip_last_error();
        return false;
    }
    *ctl = (const uint8_t *) ctl_up_.d;
    return true;
}

// The state of an output stage, N values of type T per stream (level_state, limiter_state, comfort_state): on the handle's current stream
// behind everything enqueued.  A handle that never used the stage answers `fresh` at once and allocates nothing to say so.
template <class T, int N>
Status Engine::stage_state(bool set, int count, const int32_t *streams, T *state, const T (&fresh)[N], T *Engine::*dev, bool (Engine::*ready)(std::string *),
                           std::string *err) {
    const Status listed = check_stream_list(count, streams, nullptr, err);
    if (listed != Status::kOk) return listed;
    if (!set && !(this->*dev)) {
        for (int i = 0; i < count; ++i) memcpy(state + (size_t) i * N, fresh, sizeof(fresh));
        return Status::kOk;
    }
    (void) hipSetDevice(device_);
    if (async_n_ && !drain_async(err)) return Status::kRuntime;
    if (!(this->*ready)(err)) return Status::kRuntime;
    std::vector<T> all((size_t) B_ * N);
    hipError_t e = hipMemcpyAsync(all.data(), this->*dev, all.size() * sizeof(T), hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    for (int i = 0; e == hipSuccess && i < count; ++i) {
        T *mine = &all[(size_t) (streams ? streams[i] : i) * N], *theirs = state + (size_t) i * N;
        memcpy(set ? mine : theirs, set ? theirs : mine, sizeof(fresh));
    }
    if (e == hipSuccess && set) {
        e = hipMemcpyAsync(this->*dev, all.data(), all.size() * sizeof(T), hipMemcpyHostToDevice, stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);  // (`all` goes out of scope)
    }
    if (e != hipSuccess) {
        (void) hipGetLastError();
        *err = hip_error(e);
        return Status::kRuntime;
    }
    return Status::kOk;
}

// ------------------------------------------------------------------------------------------------ output leveller

// Output leveller (StreamOptions::level): every buffer of the feature at first use -- by a call that levels or by level_state -- all or
// nothing; the state begins fresh, cleared on the handle's stream.
bool Engine::level_ready(std::string *err) {
    if (d_lv_state_) return true;
    (void) hipSetDevice(device_);
    const bool tables = table_alloc(&lv_tab_, sizeof(LevelSetting)) && ctl_ready();
    if (tables && !d_lv_gains_) d_lv_gains_ = (float *) dalloc((size_t) B_ * Tmax_ * 8, false);
    if (tables && !d_lv_rep_) d_lv_rep_ = (float *) dalloc((size_t) B_ * Tmax_ * 16, false);
    float *state = tables && d_lv_gains_ && d_lv_rep_ ? (float *) dalloc((size_t) Bpad_ * 8, false) : nullptr;
    if (!state) {
        (void) hipGetLastError();
        *err = "Failed to allocate the buffers of the output leveller.";
        return false;
    }
    launch_level_reset(state, nullptr, Bpad_, stream_);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return false;
    }
    d_lv_state_ = state;
    return true;
}

// The leveller's two launches behind the kernels of a device-pointer call (run_call), under the control rows of the call's setup;
// `report` is what the call's synthesis kernels have written -- the caller's (then column 3 of a levelling stream's rows becomes its gain)
// or the engine's.  A call on which some stream limits (StreamOptions::limiter) runs the tracker only if some stream levels, and then the
// limiter's launch, which applies the ramp too, in the place of level_apply_kernel.
bool Engine::run_level(const Call &c, const float *report, bool callers_report, const CallSetup &setup, std::string *err) {
    LevelArgs a;
    a.set = (const LevelSetting *) lv_tab_.up.d, a.state = d_lv_state_, a.ctl = setup.ctl;
    a.report = report, a.report_out = callers_report ? (float *) report : nullptr;
    a.gains = d_lv_gains_, a.out = c.out;
    a.B = B_, a.T = c.T;
    if (!(setup.stages & kStageLimiter)) {
        launch_level(a, stream_);
    } else {
        if (setup.stages & kStageLevel) launch_level_track(a, stream_);
        LimitArgs m;
        m.set = (const LimiterSetting *) lm_tab_.up.d, m.state = d_lm_state_, m.ctl = setup.ctl;
        m.gains = setup.stages & kStageLevel ? d_lv_gains_ : nullptr, m.out = c.out;
        m.B = B_, m.T = c.T;
        launch_limit(m, stream_);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return false;
    }
    return true;
}

Status Engine::level_state(bool set, int count, const int32_t *streams, float *state, std::string *err) {
    static const float fresh[2] = {0.0f, 1.0f};  // lvl, gain
    return stage_state(set, count, streams, state, fresh, &Engine::d_lv_state_, &Engine::level_ready, err);
}

// ------------------------------------------------------------------------------------------------ peak limiter

// Peak limiter (StreamOptions::limiter): every buffer of the feature at first use -- by a call that limits or by limiter_state -- all or
// nothing, the leveller's among them (the limiter's launch reads its gain pairs); g begins at 1, set on the handle's stream.
bool Engine::limiter_ready(std::string *err) {
    if (d_lm_state_) return true;
    if (!level_ready(err)) return false;
    (void) hipSetDevice(device_);
    float *state = table_alloc(&lm_tab_, sizeof(LimiterSetting)) ? (float *) dalloc((size_t) Bpad_ * 4, false) : nullptr;
    if (!state) {
        (void) hipGetLastError();
        *err = "Failed to allocate the buffers of the peak limiter.";
        return false;
    }
    launch_limit_reset(state, nullptr, Bpad_, stream_);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return false;
    }
    d_lm_state_ = state;
    return true;
}

Status Engine::limiter_state(bool set, int count, const int32_t *streams, float *state, std::string *err) {
    static const float fresh[1] = {1.0f};  // g
    return stage_state(set, count, streams, state, fresh, &Engine::d_lm_state_, &Engine::limiter_ready, err);
}

// ------------------------------------------------------------------------------------------------ comfort noise

// Comfort noise (StreamOptions::comfort): every buffer of the feature at first use -- by a call with some stream's comfort noise on or by
// comfort_state -- all or nothing; the counters begin at 0, cleared on the handle's stream.  (d_cf_n_ is not zeroed: comfort_count_kernel
// writes every row of a call's counter values on the call's stream in front of the kernels that read them.)
bool Engine::comfort_ready(std::string *err) {
    if (d_cf_state_) return true;
    (void) hipSetDevice(device_);
    const bool tables = table_alloc(&cf_tab_, sizeof(ComfortSetting)) && table_alloc(&cfa_tab_, (size_t) kComfortRow * 4) && ctl_ready();
    if (tables && !d_cf_n_) d_cf_n_ = (uint32_t *) dalloc((size_t) Bpad_ * Tmax_ * 4, false);
    uint32_t *state = tables && d_cf_n_ ? (uint32_t *) dalloc((size_t) Bpad_ * 4, false) : nullptr;
    if (!state) {
        (void) hipGetLastError();
        *err = "Failed to allocate the buffers of the comfort noise.";
        return false;
    }
    launch_comfort_reset(state, nullptr, Bpad_, stream_);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return false;
    }
    d_cf_state_ = state;
    return true;
}

// The counter's launch in front of the kernels of a device-pointer call (run_call), under the control rows of the call's setup.
bool Engine::run_comfort(const Call &c, const CallSetup &setup, std::string *err) {
    ComfortArgs a;
    a.set = setup.comfort_set, a.state = d_cf_state_, a.ctl = setup.ctl, a.n = d_cf_n_;
    a.B = B_, a.Bpad = Bpad_, a.T = c.T;
    launch_comfort(a, stream_);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return false;
    }
    return true;
}

Status Engine::comfort_state(bool set, int count, const int32_t *streams, uint32_t *n, std::string *err) {
    static const uint32_t fresh[1] = {0u};
    return stage_state(set, count, streams, n, fresh, &Engine::d_cf_state_, &Engine::comfort_ready, err);
}

// ------------------------------------------------------------------------------------------------ stream records

namespace {
struct StateHeader {  // the first 32 bytes of a record (kns_kernels.h)
    uint32_t magic, version, front_taps, precision;
    uint64_t model;
    uint32_t sample_rate;  // version 2 (handles that are not at 16 kHz); version 1: reserved, zero
    uint32_t reserved;
};
static_assert(sizeof(StateHeader) == kStateHeaderBytes, "record header");
}  // namespace

bool Engine::state_ready(std::string *err) {
    if (d_state_) return true;
    (void) hipSetDevice(device_);
    // (the records' version-1 part and the sample-rate stages' part are staged apart: the state kernels see the records they always saw)
    bool ok = recof_up_.ready(this, (size_t) Bpad_ * 4);
    if (ok && rate_ != kRate16k && !d_state_rs_) d_state_rs_ = (uint8_t *) dalloc((size_t) B_ * rs_record_bytes(rate_), false);
    ok = ok && (rate_ == kRate16k || d_state_rs_);
    if (ok && pk_max_ && !d_state_pk_) d_state_pk_ = (uint8_t *) dalloc((size_t) B_ * pk_record_bytes(rate_), false);
    ok = ok && (!pk_max_ || d_state_pk_);
    uint8_t *d = ok ? (uint8_t *) dalloc((size_t) B_ * state_record_bytes(taps_), false) : nullptr;
    if (!d) {
        // (what was allocated stays on the handle's lists and goes with the handle; the next call tries the rest again)
        (void) hipGetLastError();
        *err = "Failed to allocate the staging buffers of stream records.";
        return false;
    }
    d_state_ = d;
    return true;
}

// Checks a stream list (nullptr: 0 .. count - 1); state_list uploads its inverse -- stream -> record, -1 = not listed -- on the handle's stream.
Status Engine::check_stream_list(int count, const int32_t *streams, std::vector<int32_t> *inv, std::string *err) const {
    if (count < 1 || count > B_) {
        *err = "`count` " + std::to_string(count) + " is outside [1, " + std::to_string(B_) + "].";
        return Status::kBadArgument;
    }
    std::vector<int32_t> mine;
    if (!inv) inv = &mine;
    inv->assign((size_t) Bpad_, -1);
    for (int i = 0; i < count; ++i) {
        const int b = streams ? streams[i] : i;
        if (b < 0 || b >= B_) {
            *err = "`streams[" + std::to_string(i) + "]` = " + std::to_string(b) + " is outside [0, " + std::to_string(B_) + ").";
            return Status::kBadArgument;
        }
        if ((*inv)[b] >= 0) {  // (refused for export too: one stream -> record table serves both directions)
            *err = "`streams[" + std::to_string(i) + "]`: slot " + std::to_string(b) + " is listed twice.";
            return Status::kBadArgument;
        }
        (*inv)[b] = i;
    }
    return Status::kOk;
}

Status Engine::state_list(int count, const int32_t *streams, std::string *err) {
    std::vector<int32_t> inv;
    const Status listed = check_stream_list(count, streams, &inv, err);
    if (listed != Status::kOk) return listed;
    if (!state_ready(err)) return Status::kRuntime;
    int k;
    void *slot = recof_up_.take(&k);
    if (slot) memcpy(slot, inv.data(), (size_t) Bpad_ * 4);
    if (!slot || !recof_up_.send(k, (size_t) Bpad_ * 4, stream_)) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    return Status::kOk;
}

StateArgs Engine::state_args() const {
    StateArgs a;
    a.hist[0] = d_hist_[hist_cur_], a.hist[1] = d_hist_[hist_cur_ ^ 1];
    a.tail[0] = d_tail_[tail_cur_], a.tail[1] = d_tail_[tail_cur_ ^ 1];
    a.hstate[0] = d_hstate_[hs_cur_], a.hstate[1] = d_hstate_[hs_cur_ ^ 1];
    a.fhist = d_fhist_;
    a.rec_of = (const int32_t *) recof_up_.d;
    a.records = d_state_;
    const StateHeader h{kStateMagic, pk_max_ ? kStateVersionPacket : rate_ == kRate16k ? kStateVersion : kStateVersionRate, (uint32_t) taps_,
                        (uint32_t) prec_, model_key_, rate_ == kRate16k && !pk_max_ ? 0u : (uint32_t) rate_, 0};
    memcpy(&a.hdr0, &h, 16);
    memcpy(&a.hdr1, (const char *) &h + 16, 16);
    a.state_bytes = (uint32_t) state_record_bytes(taps_);
    a.Bpad = Bpad_;
    a.nbf = nbf_;
    a.precision = prec_;
    a.taps = taps_;
    return a;
}

void Engine::launch_states(bool import, bool packet_part) {
    if (import) launch_state_import(state_args(), stream_);
    else launch_state_export(state_args(), stream_);
    if (pk_max_ && packet_part) {
        PacketStateArgs a = packet_state_args();
        a.import = import ? 1 : 0;
        launch_packet_state(a, stream_);
    }
    if (rate_ == kRate16k) return;
    ResampleStateArgs a;
    for (int c = 0; c < 2; ++c) a.state_in[c] = d_rs_state_[0][rs_cur_ ^ c], a.state_out[c] = d_rs_state_[1][rs_cur_ ^ c];
    a.hist_in = rs_in_hist(rate_), a.hist_out = rs_out_hist(rate_);
    a.rec_of = (const int32_t *) recof_up_.d;
    a.records = d_state_rs_;
    a.rec_bytes = (uint32_t) rs_record_bytes(rate_);
    a.Bpad = Bpad_;
    a.import = import ? 1 : 0;
    launch_resample_state(a, stream_);
}

Status Engine::export_state(int count, const int32_t *streams, void *host_records, std::string *err) {
    (void) hipSetDevice(device_);
    if (async_n_ && !drain_async(err)) return Status::kRuntime;
    const Status listed = state_list(count, streams, err);
    if (listed != Status::kOk) return listed;
    launch_states(false, true);
    hipError_t e = hipGetLastError();
    const size_t S = state_bytes(), S1 = state_record_bytes(taps_), S2 = rate_ == kRate16k ? 0 : rs_record_bytes(rate_), S3 = S - S1 - S2;
    if (e == hipSuccess && S == S1) e = hipMemcpyAsync(host_records, d_state_, (size_t) count * S, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess && S > S1) e = hipMemcpy2DAsync(host_records, S, d_state_, S1, S1, (size_t) count, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess && S2)
        e = hipMemcpy2DAsync((char *) host_records + S1, S, d_state_rs_, S2, S2, (size_t) count, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess && S3)  // (a packet handle's part)
        e = hipMemcpy2DAsync((char *) host_records + S1 + S2, S, d_state_pk_, S3, S3, (size_t) count, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        *err = hip_error(e);
        return Status::kRuntime;
    }
    return Status::kOk;
}

Status Engine::import_state(int count, const int32_t *streams, const void *host_records, std::string *err) {
    (void) hipSetDevice(device_);
    if (async_n_ && !drain_async(err)) return Status::kRuntime;
    // every header before anything is written (the list is checked by state_list, which writes only the table)
    const size_t S = state_bytes(), S1 = state_record_bytes(taps_), S2 = rate_ == kRate16k ? 0 : rs_record_bytes(rate_), S3 = S - S1 - S2;
    const uint32_t want_version = pk_max_ ? kStateVersionPacket : rate_ == kRate16k ? kStateVersion : kStateVersionRate;
    for (int i = 0; i < count && count <= B_; ++i) {
        StateHeader h;
        memcpy(&h, (const char *) host_records + (size_t) i * S, sizeof(h));
        std::string what;
        if (h.magic != kStateMagic) what = "magic is not `KNSS`";
        else if (h.version != want_version) what = "version " + std::to_string(h.version) + " is not " + std::to_string(want_version);
        else if (h.front_taps != (uint32_t) taps_)
            what = "front_taps " + std::to_string(h.front_taps) + " does not match the handle's model (" + std::to_string(taps_) + ")";
        else if (h.precision != (uint32_t) prec_)
            what = std::string("precision is ") + (h.precision == kBf16 ? "bf16" : h.precision == kFp32 ? "fp32" : "unknown") +
                   ", the handle's is " + (prec_ == kBf16 ? "bf16" : "fp32") + " (records do not cross precisions)";
        else if (h.model != model_key_) what = "model hash does not match the handle's model";
        else if ((rate_ != kRate16k || pk_max_) && h.sample_rate != (uint32_t) rate_)
            what = "sample_rate " + std::to_string(h.sample_rate) + " is not the handle's (" + std::to_string(rate_) + ")";
        else if (pk_max_) {
            uint32_t fill;
            memcpy(&fill, (const char *) host_records + (size_t) i * S + S1 + S2, 4);
            if (fill >= (uint32_t) rs_frame_length(rate_))
                what = "fill " + std::to_string(fill) + " is not below the frame length " + std::to_string(rs_frame_length(rate_));
        }
        if (!what.empty()) {
            *err = "record " + std::to_string(i) + ": " + what + ".";
            return Status::kBadArgument;
        }
    }
    const Status listed = state_list(count, streams, err);
    if (listed != Status::kOk) return listed;
    // (a version-2 record interleaves the two staged parts)
    hipError_t e = S == S1 ? hipMemcpyAsync(d_state_, host_records, (size_t) count * S, hipMemcpyHostToDevice, stream_)
                           : hipMemcpy2DAsync(d_state_, S1, host_records, S, S1, (size_t) count, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess && S2)
        e = hipMemcpy2DAsync(d_state_rs_, S2, (const char *) host_records + S1, S, S2, (size_t) count, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess && S3)
        e = hipMemcpy2DAsync(d_state_pk_, S3, (const char *) host_records + S1 + S2, S, S3, (size_t) count, hipMemcpyHostToDevice, stream_);
    if (e == hipSuccess) {
        launch_states(true, true);
        e = hipGetLastError();
    }
    // (the copy may read pageable records when it runs, not when it is enqueued: the call returns once the stream has passed it)
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        *err = hip_error(e);
        return Status::kRuntime;
    }
    for (int i = 0; pk_max_ && i < count; ++i) {  // the host mirror of fill follows the records
        uint32_t fill;
        memcpy(&fill, (const char *) host_records + (size_t) i * S + S1 + S2, 4);
        pk_fill_[streams ? streams[i] : i] = (int32_t) fill;
    }
    return Status::kOk;
}

// ------------------------------------------------------------------------------------------------ the host-pointer boundary

// Handles that are not the plain one -- a rate other than 16 kHz, a packet handle, a sample format -- meet host memory HERE and nowhere
// else: the two public entries (process, run_packets) decide every refusal in pure host code, copy the caller's input into the one staging
// buffer, run the layers below on device pointers (format stage, packetiser, held streams, rate stages, run_call), copy the result back
// and wait.  The plain handle's host calls are run_call's own (sub-chunks, one-frame graph).

// Host or device memory of a call's three buffers; false and *err where the kinds are mixed (the entry maps the status).
static bool call_on_host(const void *pcm, const void *out, const void *report, bool *host, std::string *err) {
    *host = pointer_kind(pcm) != kPtrDevice;
    if ((pointer_kind(out) != kPtrDevice) != *host) {
        *err = "`pcm` and `enhanced` must both be host or both be device memory.";
        return false;
    }
    if (report && (pointer_kind(report) != kPtrDevice) != *host) {
        *err = "`report` must be memory of the same kind as `enhanced`: host with host, device with device.";
        return false;
    }
    return true;
}

// The one copy of caller host memory to the device: `bytes` of `pcm` into d_host_io_ [B][io_row()] elements of the handle's format (and
// d_host_rep_ [B][Tmax][4] for a call with a report), both allocated by the first call that needs them.
bool Engine::stage_in(const void *pcm, size_t bytes, bool report, std::string *err) {
    if (!d_host_io_) d_host_io_ = (uint8_t *) dalloc((size_t) B_ * io_row() * sample_bytes(), false);
    if (report && !d_host_rep_) d_host_rep_ = (float *) dalloc((size_t) B_ * Tmax_ * 16, false);
    if (!d_host_io_ || (report && !d_host_rep_)) {
        (void) hipGetLastError();
        *err = "Failed to allocate the staging buffer of host-memory calls.";
        return false;
    }
    if (bytes && hipMemcpyAsync(d_host_io_, pcm, bytes, hipMemcpyHostToDevice, stream_) != hipSuccess) {
        *err = hip_last_error();
        return false;
    }
    return true;
}

// ... and the one copy back, then the wait: a frame call's straight into the caller's memory, a packet call's into host_out_ / host_rep_.
bool Engine::stage_out(void *out, size_t bytes, float *report, size_t report_bytes, std::string *err) {
    hipError_t e = bytes ? hipMemcpyAsync(out, d_host_io_, bytes, hipMemcpyDeviceToHost, stream_) : hipSuccess;
    if (e == hipSuccess && report_bytes) e = hipMemcpyAsync(report, d_host_rep_, report_bytes, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        *err = hip_error(e);
        return false;
    }
    return true;
}

// One frame call.  The refusals stand in front of everything that is enqueued, in the order an S16 handle has always reported them (a
// format handle used to report the pointer kinds first): held streams with resets, pointer kinds, late resets of a several-frame
// front-end.  What can fail behind them is HIP.  On a format handle format_in_kernel takes the call's elements to int16 (d_fmt_in_), the
// S16 call runs from d_fmt_in_ to d_fmt_out_, and format_out_kernel takes the result to the caller's elements (kns_format.hip); the input is
// consumed before the output is written, so `pcm` and `enhanced` may overlap in any way.
Status Engine::process(const Call &c, std::string *err) {
    if (c.hold && c.resets) {
        *err = "held streams are not combined with per-frame stream resets in one call.";
        return Status::kBadArgument;
    }
    if (c.opt.channel_link) {  // linked channels: the handle, the table the linked kernels read, and a group that is held as a whole or not at all
        if (!channel_link_ok(ch_)) {
            *err = "linked channels need a handle whose `channels` is 2, 4 or 8 (this handle's `channels` = " + std::to_string(ch_) + ").";
            return Status::kBadArgument;
        }
        if (!c.opt.min_gain) {
            *err = "a linked call carries the handle's minimum gains (all zero where no limit is in force).";
            return Status::kBadArgument;
        }
        for (int b = 0; c.hold && b < B_; ++b) {
            const int first = b - b % ch_;
            if ((c.hold[b] != 0) != (c.hold[first] != 0)) {
                *err = "`hold[" + std::to_string(b) + "]` = " + std::to_string((int) c.hold[b]) + " differs from `hold[" + std::to_string(first) + "]` = " +
                       std::to_string((int) c.hold[first]) + ": streams " + std::to_string(first) + " and " + std::to_string(b) + " are channels of group " +
                       std::to_string(b / ch_) + ", whose masks are linked (`channels` = " + std::to_string(ch_) + "): a group is held as a whole.";
                return Status::kBadArgument;
            }
        }
    }
    if (c.high_band) {  // high-band carry: the handle, and what the feature does not take yet (the owner refuses all of it by name first)
        if (!hb_rate_ok(rate_) || pk_max_) {
            *err = "the high-band carry needs a frame handle whose `sample_rate` is 32000 or 48000.";
            return Status::kBadArgument;
        }
        bool held = false, late = false;
        for (int b = 0; c.hold && b < B_ && !held; ++b) held = c.hold[b] != 0;
        for (size_t i = 0; c.resets && i < (size_t) B_ * c.T && !late; ++i) late = c.resets[i] != 0 && i % (size_t) c.T != 0;
        if (held || late) {
            *err = held ? "`hold` is not available yet while the high-band carry is on." :
                          "per-frame stream resets after frame 0 are not available yet while the high-band carry is on.";
            return Status::kBadArgument;
        }
    }
    // the output stages: what they are not combined with yet (the owner refuses all of it by name first)
    for (const OutputStage &s : output_stages()) {
        if (!s.on(c.opt)) continue;
        if (c.opt.channel_link || c.high_band || fr_rate_) {
            *err = std::string(s.name) + (c.opt.channel_link ? " is not available yet while the channel link is on." :
                                          c.high_band        ? " is not available yet while the high-band carry is on." :
                                                               " is not available yet on a handle at 44100 or 22050 Hz.");
            return Status::kBadArgument;
        }
        if (s.carries_profile && (!c.opt.comfort_amp || !c.opt.band_profile)) {
            *err = std::string(s.call) + " carries the amplitude table and the handle's band profile (neutral where none is in force).";
            return Status::kBadArgument;
        }
    }
    // the plain handle -- but for a levelling call on host memory, which goes through the boundary below: one copy in, the device route and
    // the leveller's launches behind it, one copy out (not the sub-chunk pipeline nor the one-frame graph, which end in host memory)
    if (rate_ == kRate16k && fmt_ == kFmtS16 && ch_ == 1 && !((c.opt.level || c.opt.limiter || c.opt.comfort) && (c.host_contract || pointer_kind(c.pcm) != kPtrDevice))) return process_frames(c, err);  // (peak limiter, comfort noise: as the leveller)
    (void) hipSetDevice(device_);
    bool host, late = false;
    if (!call_on_host(c.pcm, c.out, c.report, &host, err)) return Status::kRuntime;
    for (int b = 0; c.resets && taps_ > 1 && b < B_ && !late; ++b)
        for (int t = 1; t < c.T && !late; ++t) late = c.resets[(size_t) b * c.T + t] != 0;
    if (late) {
        *err = "per-frame stream resets after frame 0 are not supported for models with a several-frame front-end (front_taps > 1).";
        return Status::kRuntime;
    }
    const size_t n = (size_t) B_ * c.T * rs_frame_length(rate_), bytes = n * sample_bytes();
    Call dev = c;  // the call below the boundary (Call::pcm / out: elements of the handle's format behind the int16 type)
    dev.host_contract = false;
    if (host) {
        if (!stage_in(c.pcm, bytes, c.report != nullptr, err)) return Status::kRuntime;
        dev.pcm = dev.out = (int16_t *) d_host_io_;
        if (c.report) dev.report = d_host_rep_;
    }
    hipError_t e = hipSuccess;
    // channels, outermost: the call's interleaved elements are split into the rows d_ch_, on which everything below runs in place, and the
    // rows are joined into the call's output last
    const ChannelArgs split{dev.pcm, d_ch_, nullptr, (long long) c.T * rs_frame_length(rate_), B_ / ch_, ch_};
    const ChannelArgs join{d_ch_, dev.out, nullptr, split.n, split.G, ch_};
    if (ch_ > 1) {
        dev.pcm = dev.out = (int16_t *) d_ch_;
        launch_channels_split(sample_bytes(), split, stream_);
        e = hipGetLastError();
    }
    Call inner = dev;
    if (e == hipSuccess && fmt_ != kFmtS16) {
        inner.pcm = d_fmt_in_, inner.out = d_fmt_out_;
        launch_format_in(fmt_, FormatArgs{dev.pcm, d_fmt_in_, nullptr, (long long) n, 1}, stream_);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        const Status st = process_frames(inner, err);
        if (st != Status::kOk) return st;
    }
    if (e == hipSuccess && fmt_ != kFmtS16) {
        launch_format_out(fmt_, FormatArgs{d_fmt_out_, dev.out, nullptr, (long long) n, 1}, stream_);
        e = hipGetLastError();
    }
    if (e == hipSuccess && ch_ > 1) {
        launch_channels_join(sample_bytes(), join, stream_);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        *err = hip_error(e);
        return Status::kRuntime;
    }
    if (host && !stage_out(c.out, bytes, c.report, c.report ? (size_t) B_ * c.T * 16 : 0, err)) return Status::kRuntime;
    return Status::kOk;
}

// A call and its held streams: export the held rows' records to the device scratch, run the call unchanged, import them back -- around the
// WHOLE call (outside the one-frame graph and the sub-chunks of large host calls), all on the handle's stream, so a device-pointer call
// stays enqueued without a host wait.  The import restores both ping-pong copies, whichever parity the call has left current.
Status Engine::process_frames(const Call &c, std::string *err) {
    std::vector<int32_t> held;
    for (int b = 0; c.hold && b < B_; ++b)
        if (c.hold[b]) held.push_back(b);
    if (held.empty()) return advance(c, err) ? Status::kOk : Status::kRuntime;
    (void) hipSetDevice(device_);
    if (async_n_ && !drain_async(err)) return Status::kRuntime;
    const Status listed = state_list((int) held.size(), held.data(), err);
    if (listed != Status::kOk) return listed;
    launch_states(false, false);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return Status::kRuntime;
    }
    if (!advance(c, err)) return Status::kRuntime;  // (a refused call has advanced nothing)
    launch_states(true, false);
    e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hip_error(e);
        return Status::kRuntime;
    }
    return Status::kOk;
}

// ------------------------------------------------------------------------------------------------ packet handles

bool Engine::enable_packets(int max_samples, std::string *err) {
    (void) hipSetDevice(device_);
    const int F = rs_frame_length(rate_);
    // a stream completes at most floor((F - 1 + max_samples) / F) = ceil(max_samples / F) = Tmax frames in a call
    const size_t K = (size_t) Tmax_;
    const size_t tab_bytes = ((size_t) Bpad_ + 2 + K) * 4 + (size_t) Bpad_;  // counts, the number of sub-calls, <= K + 1 cuts; the mask
    d_pk_pin_ = (int16_t *) dalloc((size_t) Bpad_ * F * 2, true);
    d_pk_pout_ = (int16_t *) dalloc((size_t) Bpad_ * F * 2, true);
    d_pk_fill_[0] = (int32_t *) dalloc((size_t) Bpad_ * 4, true);
    d_pk_fill_[1] = (int32_t *) dalloc((size_t) Bpad_ * 4, true);
    d_pk_in_ = (int16_t *) dalloc((size_t) B_ * K * F * 2, false);
    d_pk_out_ = (int16_t *) dalloc((size_t) B_ * K * F * 2, false);
    d_pk_rep_ = (float *) dalloc((size_t) B_ * K * 16, false);
    if (!d_pk_pin_ || !d_pk_pout_ || !d_pk_fill_[0] || !d_pk_fill_[1] || !d_pk_in_ || !d_pk_out_ || !d_pk_rep_ ||
        !pk_up_.ready(this, tab_bytes)) {
        (void) hipGetLastError();
        *err = "Failed to allocate the buffers of a packet handle.";
        return false;
    }
    pk_fill_.assign((size_t) B_, 0);
    pk_max_ = max_samples;
    return true;
}

PacketStateArgs Engine::packet_state_args() const {
    PacketStateArgs a;
    a.pin = d_pk_pin_, a.pout = d_pk_pout_;
    a.fill_in = d_pk_fill_[0], a.fill_out = d_pk_fill_[1];
    a.rec_of = (const int32_t *) recof_up_.d;
    a.records = d_state_pk_;
    a.rec_bytes = (uint32_t) pk_record_bytes(rate_);
    a.Bpad = Bpad_, a.F = rs_frame_length(rate_), a.import = 0;
    return a;
}

// One call of a packet handle (fourth extension; section 6).  The plan is made on the host from the mirror of fill:
// stream b completes k_b = (fill_b + counts[b]) / F frames; the sub-calls are cut at every distinct non-zero k_b (k_b <= max_frames always), and
// sub-call [c0, c1) holds the streams with k_b < c1 (koala_amd/packets.py restates the plan).  Every refusal is decided before anything is
// touched: max_samples, counts, report_frames, pointer kinds.  Then everything goes onto the handle's stream: on a format handle
// format_in_kernel over the whole rows [B][max_samples] (the caller owns them), the call's table, the masked reset of `restart`,
// packet_in_kernel, the sub-calls through process_frames -- routes, held streams, rate stages, attenuation limit and report as they are --
// packet_out_kernel, and on a format handle format_out_kernel, which writes row b's first counts[b] elements only, from the call's table
// (pk_up_'s starts with the counts).  A call without a sample (restarts only) moves and converts no samples.  Host pointers: the staging
// stands in for the caller's device memory, and of what comes back only a row's first counts[b] elements and a stream's first k_b report
// rows are copied on: the rest of the caller's bytes stay.
Status Engine::run_packets(const PacketCall &c, std::string *err) { return fr_rate_ ? run_fractional(c, err) : run_packet_call(c, fmt_, ch_, err); }

// ---- what the two packet calls (run_packet_call, run_fractional) share: the refusals, and the caller's side of the call

// `max_samples` and `counts`, the first two refusals -- on a handle with channels (ch > 1) the streams of a group share a row, so their
// counts must be equal; what the call holds at all
Status Engine::packet_check(const PacketCall &c, int most, int ch, bool *any_restart, bool *any_count, std::string *err) const {
    if (c.max_samples < 1 || c.max_samples > most) {
        *err = "`max_samples` " + std::to_string(c.max_samples) + " is outside [1, " + std::to_string(most) + "].";
        return Status::kBadArgument;
    }
    *any_restart = *any_count = false;
    for (int b = 0; b < B_; ++b) {
        if (c.counts[b] < 0 || c.counts[b] > c.max_samples) {
            *err = "`counts[" + std::to_string(b) + "]` = " + std::to_string(c.counts[b]) + " is outside [0, " + std::to_string(c.max_samples) + "].";
            return Status::kBadArgument;
        }
        *any_restart = *any_restart || (c.restart && c.restart[b]);
        *any_count = *any_count || c.counts[b] > 0;
    }
    for (int b = 0; ch > 1 && b < B_; ++b) {
        const int first = b - b % ch;
        if (c.counts[b] != c.counts[first]) {
            *err = "`counts[" + std::to_string(b) + "]` = " + std::to_string(c.counts[b]) + " differs from `counts[" + std::to_string(first) + "]` = " +
                   std::to_string(c.counts[first]) + ": streams " + std::to_string(first) + " and " + std::to_string(b) + " are channels of group " +
                   std::to_string(b / ch) + ", whose samples share a row (`channels` = " + std::to_string(ch) + ").";
            return Status::kBadArgument;
        }
    }
    // linked channels (ch_: the handle's, also in a fractional handle's inner call): the sub-calls hold the streams by their frame count, so a
    // group's streams must complete the same frames -- equal `restart`, equal phase (the mirrors of fill and, at 44.1 / 22.05 kHz, N mod 441)
    if (c.opt.channel_link && (!channel_link_ok(ch_) || !c.opt.min_gain)) {
        *err = !c.opt.min_gain ? "a linked call carries the handle's minimum gains (all zero where no limit is in force)."
                           : "linked channels need a handle whose `channels` is 2, 4 or 8 (this handle's `channels` = " + std::to_string(ch_) + ").";
        return Status::kBadArgument;
    }
    for (int b = 0; c.opt.channel_link && b < B_; ++b) {
        const int first = b - b % ch_;
        const std::string who = ": streams " + std::to_string(first) + " and " + std::to_string(b) + " are channels of group " + std::to_string(b / ch_) +
                                ", whose masks are linked (`channels` = " + std::to_string(ch_) + ")";
        const int rb = c.restart && c.restart[b] ? 1 : 0, rf = c.restart && c.restart[first] ? 1 : 0;
        if (rb != rf) {
            *err = "`restart[" + std::to_string(b) + "]` = " + std::to_string(rb) + " differs from `restart[" + std::to_string(first) + "]` = " +
                   std::to_string(rf) + who + ": a group restarts as a whole.";
            return Status::kBadArgument;
        }
        if (rb) continue;  // (fresh before this packet: phase 0, both)
        if (pk_fill_[b] != pk_fill_[first] || (fr_rate_ && fr_phase_[b] != fr_phase_[first])) {
            *err = "group " + std::to_string(b / ch_) + " is out of phase" + who + ", and stream " + std::to_string(b) + " holds " +
                   std::to_string(pk_fill_[b]) + " samples of an unfinished frame where stream " + std::to_string(first) + " holds " +
                   std::to_string(pk_fill_[first]) + (fr_rate_ ? " (or their positions in the 441-sample period differ)" : "") +
                   ": reset or import the whole group.";
            return Status::kBadArgument;
        }
    }
    return Status::kOk;
}

// The other refusals (`report_frames` against the kmax frames a stream completes, pointer kinds), the call without a sample or a restart
// (*nothing: done, every stream stalled), then the caller's samples onto the device: host pointers are staged, and on a handle with a format
// (fmt: kFmtS16 for none, and for the inner call of a fractional handle) format_in_kernel runs over the whole rows [B][max_samples] (the
// caller owns them).  Channels (ch > 1), outermost: the whole group rows [B / ch][max_samples ch] are split into d_ch_ first, which then
// stands in for both of the caller's buffers.  io: what the call's kernels read and write from here on.
Status Engine::packet_begin(const PacketCall &c, int fmt, int ch, int kmax, bool any_restart, bool any_count, PacketIo *io, bool *nothing, std::string *err) {
    *nothing = false;
    if (c.report && c.report_frames < kmax) {
        *err = "`report_frames` " + std::to_string(c.report_frames) + " is below the " + std::to_string(kmax) + " frames a stream completes in this call.";
        return Status::kBadArgument;
    }
    (void) hipSetDevice(device_);
    if (!call_on_host(c.pcm, c.out, c.report, &io->host, err)) return Status::kBadArgument;
    if (!any_count && !any_restart) {  // every stream stalled: nothing to do
        for (int b = 0; c.frames && b < B_; ++b) c.frames[b] = 0;
        *nothing = true;
        return Status::kOk;
    }
    io->convert = fmt != kFmtS16 && any_count;
    io->bytes = any_count ? (size_t) B_ * c.max_samples * fmt_bytes(fmt) : 0;
    // what the call reads and writes on the device: the caller's memory, or the staging (its report rows kmax apart)
    const void *src = c.pcm;
    io->dst = c.out;
    io->report = c.report;
    io->report_frames = c.report_frames;
    if (io->host) {
        if (!stage_in(c.pcm, io->bytes, c.report != nullptr, err)) return Status::kRuntime;
        src = io->dst = d_host_io_;
        if (c.report) io->report = d_host_rep_, io->report_frames = kmax;
    }
    io->joined = nullptr;
    if (ch > 1 && any_count) {
        launch_channels_split(fmt_bytes(fmt), ChannelArgs{src, d_ch_, nullptr, (long long) c.max_samples, B_ / ch, ch}, stream_);
        if (hipGetLastError() != hipSuccess) {
            *err = hip_last_error();
            return Status::kRuntime;
        }
        io->joined = io->dst;
        src = io->dst = d_ch_;
    }
    if (io->convert) {
        launch_format_in(fmt, FormatArgs{src, d_fmt_in_, nullptr, (long long) B_ * c.max_samples, 1}, stream_);
        if (hipGetLastError() != hipSuccess) {
            *err = hip_last_error();
            return Status::kRuntime;
        }
    }
    io->in16 = fmt != kFmtS16 ? d_fmt_in_ : (const int16_t *) src;
    io->out16 = fmt != kFmtS16 ? d_fmt_out_ : (int16_t *) io->dst;
    return Status::kOk;
}

// ... and back: format_out_kernel writes row b's first counts[b] elements only, from the call's device table (d_counts: it starts with the
// counts); of what a host call's staging brings back only a row's first counts[b] elements and a stream's first k[b] report rows are
// copied on, the rest of the caller's bytes stay.  Channels: the join writes group g's first counts[g ch] ch elements from the same table,
// and that much of a group's row is what a host call copies on.
Status Engine::packet_end(const PacketCall &c, int fmt, int ch, const PacketIo &io, const int32_t *d_counts, const int32_t *k, int kmax, std::string *err) {
    if (io.convert) launch_format_out(fmt, FormatArgs{d_fmt_out_, io.dst, d_counts, (long long) c.max_samples, B_}, stream_);
    if (io.joined) launch_channels_join(fmt_bytes(fmt), ChannelArgs{io.dst, io.joined, d_counts, (long long) c.max_samples, B_ / ch, ch}, stream_);
    if (hipGetLastError() != hipSuccess) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    if (!io.host) return Status::kOk;
    const size_t eb = (size_t) fmt_bytes(fmt), rep_floats = c.report ? (size_t) B_ * kmax * 4 : 0;
    host_out_.resize((size_t) B_ * c.max_samples * eb);
    host_rep_.resize(rep_floats);
    if (!stage_out(host_out_.data(), io.bytes, host_rep_.data(), rep_floats * 4, err)) return Status::kRuntime;
    for (int b = 0; b < B_; ++b) {
        const size_t at = (size_t) b * c.max_samples * eb;
        if (b % ch == 0) memcpy((uint8_t *) c.out + at, host_out_.data() + at, (size_t) c.counts[b] * ch * eb);  // (ch == 1: every row)
        if (c.report) memcpy(c.report + (size_t) b * c.report_frames * 4, host_rep_.data() + (size_t) b * kmax * 4, (size_t) k[b] * 16);
    }
    return Status::kOk;
}

Status Engine::run_packet_call(const PacketCall &c, int fmt, int ch, std::string *err) {
    // (the owner refuses it by name first)
    if (c.opt.channel_link && refuse_stages(c.opt, " is not available yet while the channel link is on.", err)) return Status::kBadArgument;
    const int F = rs_frame_length(rate_);
    bool any_restart, any_count, nothing;
    Status st = packet_check(c, pk_max_, ch, &any_restart, &any_count, err);
    if (st != Status::kOk) return st;
    std::vector<int32_t> k((size_t) B_);
    std::vector<int32_t> cuts{0};
    int kmax = 0;
    for (int b = 0; b < B_; ++b) {
        k[b] = ((c.restart && c.restart[b] ? 0 : pk_fill_[b]) + c.counts[b]) / F;
        kmax = std::max(kmax, k[b]);
    }
    PacketIo io;
    st = packet_begin(c, fmt, ch, kmax, any_restart, any_count, &io, &nothing, err);
    if (st != Status::kOk || nothing) return st;
    {  // the sub-calls: frames [cuts[l], cuts[l + 1])
        std::vector<int32_t> ks(k);
        std::sort(ks.begin(), ks.end());
        for (int32_t v : ks) {
            if (v > cuts.back()) cuts.push_back(v);  // (v <= Tmax: no sub-call is longer than the inner engine's max_frames)
        }
    }
    const int nsub = (int) cuts.size() - 1;
    // the call's table, and the restart mask behind it
    const size_t tab_ints = (size_t) Bpad_ + 2 + (size_t) Tmax_;
    int slot;
    int32_t *tab = (int32_t *) pk_up_.take(&slot);
    if (!tab) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    uint8_t *mask = (uint8_t *) (tab + tab_ints);
    memset(tab, 0, tab_ints * 4 + (size_t) Bpad_);
    memcpy(tab, c.counts, (size_t) B_ * 4);
    tab[Bpad_] = nsub;
    memcpy(tab + Bpad_ + 1, cuts.data(), cuts.size() * 4);
    for (int b = 0; any_restart && b < B_; ++b) mask[b] = c.restart[b] ? 1 : 0;
    if (!pk_up_.send(slot, tab_ints * 4 + (size_t) Bpad_, stream_)) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    const int32_t *d_tab = (const int32_t *) pk_up_.d;
    if (any_restart) {
        launch_resets((const uint8_t *) (d_tab + tab_ints));
        for (int b = 0; b < B_; ++b)
            if (c.restart[b]) pk_fill_[b] = 0;
    }
    PacketArgs a;
    a.user_in = io.in16;
    a.user_out = io.out16;
    a.tab = d_tab;
    a.pin = d_pk_pin_, a.pout = d_pk_pout_;
    a.fill_in = d_pk_fill_[0], a.fill_out = d_pk_fill_[1];
    a.frames = d_pk_in_;
    a.sub_report = d_pk_rep_;
    a.report = io.report;
    a.report_frames = io.report_frames;
    a.max_samples = c.max_samples, a.B = B_, a.Bpad = Bpad_, a.F = F;
    launch_packet_in(a, stream_);
    if (hipGetLastError() != hipSuccess) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    std::vector<uint8_t> hold((size_t) B_);
    for (int l = 0; l < nsub; ++l) {
        const int c0 = cuts[l], c1 = cuts[l + 1];
        bool held = false;
        for (int b = 0; b < B_; ++b) held = (hold[b] = k[b] < c1) || held;
        Call inner{c1 - c0, d_pk_in_ + (size_t) B_ * F * c0, d_pk_out_ + (size_t) B_ * F * c0};
        inner.hold = held ? hold.data() : nullptr;
        // (the link -- packet_check: a group's streams share k_b, so a sub-call holds a group as a whole; the output stages -- the sub-calls'
        // `hold` keeps a stalled stream's leveller, its limiter's g and its comfort noise's counter where they are)
        inner.opt = c.opt;
        inner.report = c.report ? d_pk_rep_ + (size_t) B_ * c0 * 4 : nullptr;
        if (process_frames(inner, err) != Status::kOk) return Status::kRuntime;
    }
    a.frames = d_pk_out_;
    launch_packet_out(a, stream_);
    if (hipGetLastError() != hipSuccess) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    for (int b = 0; b < B_; ++b) {  // (the mirror follows what is enqueued)
        pk_fill_[b] = pk_fill_[b] + c.counts[b] - k[b] * F;
        if (c.frames) c.frames[b] = k[b];
    }
    return packet_end(c, fmt, ch, io, d_tab, k.data(), kmax, err);
}

// ------------------------------------------------------------------------------------------------ packet handles at 44 100 and 22 050 Hz

// The polyphase table of a fractional stage (kns_kernels.h, FractionalArgs::taps): [tap j][phase r] = (float) (scale g[r + P j]) over the
// prototype of K = 441, built in double and rounded once; zero where the prototype has no such tap.
static std::vector<float> fr_table(int scale, int P, int taps) {
    const std::vector<double> g = rs_prototype_g(kFrDown);
    std::vector<float> h((size_t) taps * P, 0.0f);
    for (int j = 0; j < taps; ++j)
        for (int r = 0; r < P && r + P * j < kFrTaps; ++r) h[(size_t) j * P + r] = (float) (scale * g[(size_t) r + (size_t) P * j]);
    return h;
}

bool Engine::enable_fractional(int rate, int max_samples, std::string *err) {
    (void) hipSetDevice(device_);
    const int U = fr_up(rate), T = fr_in_taps(U);
    const size_t tab_bytes = (size_t) Bpad_ * 5;  // int32 counts[Bpad], uint8 restart[Bpad]
    d_fr_in_ = (int16_t *) dalloc((size_t) B_ * pk_max_ * 2, false);
    d_fr_out_ = (int16_t *) dalloc((size_t) B_ * pk_max_ * 2, false);
    d_fr_hist_[0] = (int16_t *) dalloc((size_t) Bpad_ * T * 2, true);
    d_fr_hist_[1] = (int16_t *) dalloc((size_t) Bpad_ * kFrOutHist * 2, true);
    d_fr_phase_[0] = (int32_t *) dalloc((size_t) Bpad_ * 4, true);
    d_fr_phase_[1] = (int32_t *) dalloc((size_t) Bpad_ * 4, true);
    const std::vector<float> h_in = fr_table(U, U, T), h_out = fr_table(kFrDown, kFrDown, kFrOutTaps);
    d_fr_taps_[0] = (float *) upload(h_in.data(), h_in.size() * 4);
    d_fr_taps_[1] = (float *) upload(h_out.data(), h_out.size() * 4);
    if (!d_fr_in_ || !d_fr_out_ || !d_fr_hist_[0] || !d_fr_hist_[1] || !d_fr_phase_[0] || !d_fr_phase_[1] || !d_fr_taps_[0] || !d_fr_taps_[1] ||
        !fr_up_.ready(this, tab_bytes, true)) {
        (void) hipGetLastError();
        *err = "Failed to allocate the buffers of a handle at " + std::to_string(rate) + " Hz.";
        return false;
    }
    fr_phase_.assign((size_t) B_, 0);
    fr_rate_ = rate, fr_max_ = max_samples;
    return true;
}

FractionalStateArgs Engine::fractional_state_args() const {
    return FractionalStateArgs{d_fr_hist_[0], d_fr_hist_[1], d_fr_phase_[0], d_fr_phase_[1], fr_in_taps(fr_up(fr_rate_)), Bpad_};
}

// One call of a packet handle at 44 100 or 22 050 Hz (sixth extension; section 6): the converter sits OUTSIDE the
// packetiser.  The plan is made on the host from the mirror of N mod 441: stream b feeds the inner 16 kHz packet path
// M(N + counts[b]) - M(N) samples (koala_amd/packets.py restates it), and the inner call's own plan follows from its mirror of fill.  Every
// refusal is decided before anything is touched.  Then, on the handle's stream: [format_in], the call's table, the masked reset of
// `restart` (every layer's state at once, so the inner call sees none), fractional_in_kernel, the inner packet call on device rows -- its
// report rows and frame counts are the call's -- fractional_out_kernel, [format_out].  A call in which no stream yields an inner sample
// still runs both stages: the in-stage's history and N advance, and the out-stage delivers from the inner output it holds.
Status Engine::run_fractional(const PacketCall &c, std::string *err) {
    // (the owner refuses it by name first)
    if (refuse_stages(c.opt, " is not available yet on a handle at 44100 or 22050 Hz.", err)) return Status::kBadArgument;
    const int U = fr_up(fr_rate_);
    bool any_restart, any_count, nothing;
    Status st = packet_check(c, fr_max_, ch_, &any_restart, &any_count, err);
    if (st != Status::kOk) return st;
    std::vector<int32_t> inner((size_t) B_), k((size_t) B_, 0);
    int kmax = 0;
    for (int b = 0; b < B_; ++b) {
        const bool fresh = c.restart && c.restart[b];
        const long long ph = fresh ? 0 : fr_phase_[b];
        inner[b] = (int32_t) (fr_inner(ph + c.counts[b], U) - fr_inner(ph, U));
        kmax = std::max(kmax, ((fresh ? 0 : pk_fill_[b]) + inner[b]) / kFrame);
    }
    PacketIo io;
    st = packet_begin(c, fmt_, ch_, kmax, any_restart, any_count, &io, &nothing, err);
    if (st != Status::kOk || nothing) return st;
    int slot;
    int32_t *tab = (int32_t *) fr_up_.take(&slot);
    if (!tab) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    uint8_t *mask = (uint8_t *) (tab + Bpad_);
    memset(tab, 0, (size_t) Bpad_ * 5);
    memcpy(tab, c.counts, (size_t) B_ * 4);
    for (int b = 0; any_restart && b < B_; ++b) mask[b] = c.restart[b] ? 1 : 0;
    if (!fr_up_.send(slot, (size_t) Bpad_ * 5, stream_)) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    const int32_t *d_tab = (const int32_t *) fr_up_.d;
    if (any_restart) {
        launch_resets((const uint8_t *) (d_tab + Bpad_));
        for (int b = 0; b < B_; ++b)
            if (c.restart[b]) pk_fill_[b] = 0, fr_phase_[b] = 0;
    }
    // From here on only HIP can fail, and a call that fails half-way has advanced some layers of the streams and not the others (the
    // in-stage's N mod 441 and history are ahead of the out-stage's and of the mirror): the error is reported, and the handle's streams are
    // defined again only after pv_koala_batch_reset.  The inner call's status travels on as it is.
    FractionalArgs a;
    a.in = io.in16;
    a.out = d_fr_in_;
    a.counts = d_tab;
    a.hist = d_fr_hist_[0], a.phase = d_fr_phase_[0], a.taps = d_fr_taps_[0];
    a.in_stride = c.max_samples, a.out_stride = pk_max_, a.U = U;
    launch_fractional_in(a, B_, stream_);
    if (hipGetLastError() != hipSuccess) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    // the inner call: an S16 call on device rows, without restarts (done above); its report rows and frame counts are this call's
    // (its settings: the gains, the profile and the link -- the inner call's rows are the engine's: its `ch` is 1, the link is the handle's; the
    // output stages were refused above)
    PacketCall in16{pk_max_, inner.data(), d_fr_in_, d_fr_out_, nullptr, io.report, io.report_frames, k.data(), c.opt};
    st = run_packet_call(in16, kFmtS16, 1, err);
    if (st != Status::kOk) return st;
    a.in = d_fr_out_;
    a.out = io.out16;
    a.hist = d_fr_hist_[1], a.phase = d_fr_phase_[1], a.taps = d_fr_taps_[1];
    a.in_stride = pk_max_, a.out_stride = c.max_samples;
    launch_fractional_out(a, B_, stream_);
    if (hipGetLastError() != hipSuccess) {
        *err = hip_last_error();
        return Status::kRuntime;
    }
    for (int b = 0; b < B_; ++b) {  // (the mirror follows what is enqueued)
        fr_phase_[b] = (fr_phase_[b] + c.counts[b]) % kFrDown;
        if (c.frames) c.frames[b] = k[b];
    }
    return packet_end(c, fmt_, ch_, io, d_tab, k.data(), kmax, err);
}

// ------------------------------------------------------------------------------------------------ sample formats

// A handle whose callers hold float32 or G.711 samples (fifth extension; section 6): two int16 staging matrices
// [B][io_row()], between which the S16 handle's call runs unchanged.  The two kernel launches around that call are the entries' (process,
// run_packets: the host-pointer boundary).
bool Engine::set_format(int fmt, std::string *err) {
    if (fmt == kFmtS16) return true;
    (void) hipSetDevice(device_);
    d_fmt_in_ = (int16_t *) dalloc((size_t) B_ * io_row() * 2, false);
    d_fmt_out_ = (int16_t *) dalloc((size_t) B_ * io_row() * 2, false);
    if (!d_fmt_in_ || !d_fmt_out_) {
        (void) hipGetLastError();
        *err = "Failed to allocate the staging buffers of a sample format.";
        return false;
    }
    fmt_ = fmt;
    return true;
}

// ------------------------------------------------------------------------------------------------ channels

// A handle whose callers hold the streams of a group interleaved (seventh extension; section 6): one matrix of rows
// [B][io_row()] of the handle's format elements, into which the call is split, on which it runs in place and from which it is joined.  The
// two kernel launches are the entries' (process, run_packets: the host-pointer boundary), outside the format stage.
bool Engine::enable_channels(int C, std::string *err) {
    if (C == 1) return true;
    (void) hipSetDevice(device_);
    d_ch_ = (uint8_t *) dalloc((size_t) B_ * io_row() * sample_bytes(), false);
    if (!d_ch_) {
        (void) hipGetLastError();
        *err = "Failed to allocate the rows of a handle with channels.";
        return false;
    }
    ch_ = C;
    return true;
}

// ------------------------------------------------------------------------------------------------ debug taps

static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t) (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0) {  // zero / subnormal: value = m * 2^-24
        float f = (float) m * (1.0f / 16777216.0f);
        memcpy(&u, &f, 4);
        u |= sign;
    } else if (e == 31) {
        u = sign | 0x7f800000u | (m << 13);
    } else {
        u = sign | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static float bf16_to_float(uint16_t h) {
    uint32_t u = (uint32_t) h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int64_t Engine::debug_read(int what, float *out, int64_t capacity, std::string *err) {
    (void) hipSetDevice(device_);
    if (hipStreamSynchronize(stream_) != hipSuccess) {
        *err = hip_last_error();
        return -1;
    }
    const int T = last_T_, mtb = Bpad_ / 16;
    auto fetch = [&](const void *d, size_t bytes) {
        std::vector<uint8_t> h(bytes);
        (void) hipMemcpyAsync(h.data(), d, bytes, hipMemcpyDeviceToHost, stream_);
        (void) hipStreamSynchronize(stream_);
        return h;
    };
    // logical element (row r of m-tile, k) of an A-packed buffer with nb blocks per m-tile
    auto a_at = [&](const std::vector<uint8_t> &h, size_t mtile, int nb, int r, int k) -> float {
        const size_t blk = mtile * nb + k / pi_.kb;
        const int off = pack_off(prec_, r, k % pi_.kb);
        if (prec_ == kBf16) {
            uint16_t v;
            memcpy(&v, h.data() + blk * 1024 + (size_t) off * 2, 2);
            return bf16_to_float(v);
        }
        float v;
        memcpy(&v, h.data() + blk * 1024 + (size_t) off * 4, 4);
        return v;
    };
    int64_t n = 0;
    if ((what == 0 && !feat_valid_) || (what == 2 && !mask_valid_)) {
        *err = "the last call kept this intermediate on chip (one-frame calls fuse the front-end / the mask head into the STFT "
               "launches): use the developer build with its debug-taps switch";
        return -1;
    }
    if (what == 4 && fold_) {
        *err = "this configuration forms no embedding (bf16, one-frame front-end: folded into the stage-input GEMMs)";
        return -1;
    }
    if (what == 0 || what == 4) {  // features / embedding
        const int width = what == 0 ? kBins : kHidden, nb = what == 0 ? nbf_ : nbh_;
        n = (int64_t) T * B_ * width;
        if (n > capacity) return -2;
        auto h = fetch(what == 0 ? (const char *) d_feat_ + (size_t) (taps_ - 1) * feat_frame_bytes_ : (const char *) d_e_,
                       (size_t) T * mtb * nb * 1024);
        for (int t = 0; t < T; ++t)
            for (int b = 0; b < B_; ++b)
                for (int k = 0; k < width; ++k)
                    out[((size_t) t * B_ + b) * width + k] = a_at(h, (size_t) t * mtb + b / 16, nb, b % 16, k);
    } else if (what == 1) {  // spectrum
        if (!spec_valid_) {  // multi-frame calls rebuild the spectrum from the PCM and store none
            *err = "the last call stored no spectrum (multi-frame calls recompute it): use the developer build with its "
                   "debug-taps switch";
            return -1;
        }
        n = (int64_t) T * B_ * kBins * 2;
        if (n > capacity) return -2;
        auto h = fetch(d_spec_, (size_t) T * Bpad_ * 256 * 8);
        const float *s = (const float *) h.data();
        for (int t = 0; t < T; ++t)
            for (int b = 0; b < B_; ++b) {
                const float *src = s + ((size_t) t * Bpad_ + b) * 512;
                float *dst = out + ((size_t) t * B_ + b) * kBins * 2;
                for (int k = 0; k < 256; ++k) {  // un-permute the kernels' lane order (kns_kernels.h)
                    const int c = k & 15, k2 = k >> 4, slot = ((k2 >> 1) * 16 + c) * 2 + (k2 & 1);
                    dst[2 * k] = src[2 * slot];
                    dst[2 * k + 1] = src[2 * slot + 1];
                }
                dst[512] = dst[1];  // Nyquist travels in the imaginary slot of bin 0
                dst[513] = 0.0f;
                dst[1] = 0.0f;
            }
    } else if (what == 2) {  // mask
        n = (int64_t) T * B_ * kBins;
        if (n > capacity) return -2;
        auto h = fetch(d_mask_, (size_t) T * mtb * kMaskTiles * 1024);
        const float *s = (const float *) h.data();
        const uint16_t *sh = (const uint16_t *) h.data();  // bf16 configuration: fp16 C fragments
        for (int t = 0; t < T; ++t)
            for (int b = 0; b < B_; ++b)
                for (int k = 0; k < kBins; ++k) {
                    const size_t idx = (((size_t) t * mtb + b / 16) * kMaskTiles + k / 16) * 256 + cpack_off(b % 16, k % 16);
                    out[((size_t) t * B_ + b) * kBins + k] = prec_ == kBf16 ? half_to_float(sh[idx]) : s[idx];
                }
    } else if (what == 3) {  // hidden state
        n = (int64_t) kGruLayers * B_ * kHidden;
        if (n > capacity) return -2;
        auto h = fetch(d_hstate_[hs_cur_], (size_t) kGruLayers * mtb * kUnitTiles * 1024);
        const float *s = (const float *) h.data();
        for (int l = 0; l < kGruLayers; ++l)
            for (int b = 0; b < B_; ++b)
                for (int k = 0; k < kHidden; ++k)
                    out[((size_t) l * B_ + b) * kHidden + k] =
                        s[(((size_t) l * mtb + b / 16) * kUnitTiles + k / 16) * 256 + cpack_off(b % 16, k % 16)];
#ifdef KNS_DEV
    } else if (what == 6) {  // developer build: the route of the last call (enum Route), what rode inside other launches; a reader with room
        // for six or seven values also gets the time segments of its STFT launches (four-value readers get what they always got)
        if (capacity < 4) return -2;
        out[0] = (float) last_route_;
        out[1] = feat_valid_ ? 0.0f : 1.0f;   // front-end inside the analysis launch / features rolled into the history
        out[2] = mask_valid_ ? 0.0f : 1.0f;   // mask head inside the synthesis launch
        out[3] = spec_valid_ ? 1.0f : 0.0f;   // spectrum stored (not recomputed)
        if (capacity < 6) return 4;
        out[4] = (float) last_analysis_seg_;  // frames per time segment of the last analysis launch
        out[5] = (float) last_synth_seg_;     // ... and of the last synthesis launch
        if (capacity < 7) return 6;
        out[6] = (float) last_synth_launches_;  // synthesis launches of the call: the slices of the layer pipeline, or one
        return 7;
    } else if (what == 7) {  // developer build: recurrent launches of the last call that carried their stage's narrow head
        if (capacity < 1) return -2;
        out[0] = (float) last_head_launches_;
        return 1;
#endif
    } else if (what == 5) {  // developer build: stamps of the last fused layer launch, [8 waves][4 T][8] ticks since the first one
        if (!d_qdbg_) {
            *err = "no stamps: developer build with KOALA_AMD_QUAD_DBG=<workgroup>";
            return -1;
        }
        n = (int64_t) 8 * 4 * T * 8;
        if (n > capacity) return -2;
        auto h = fetch(d_qdbg_, (size_t) n * 8);
        const unsigned long long *st = (const unsigned long long *) h.data();
        unsigned long long t0 = ~0ull;
        for (int64_t i = 0; i < n; ++i)
            if (i % 8 < 6 && st[i] && st[i] < t0) t0 = st[i];
        // slots 0..5: ticks since the first stamp; slot 6: a 32-bit mask as two 16-bit halves is too wide for a float -- split
        // below; slot 7: a small count
        for (int64_t i = 0; i < n; ++i)
            out[i] = i % 8 == 7 ? (float) (st[i] & 0xffff) + 65536.0f * (float) (st[i - 1] >> 16 & 0xffff)  // count + mask's high half
                     : i % 8 == 6 ? (float) (st[i] & 0xffff)
                                  : (st[i] ? (float) (st[i] - t0) : -1.0f);
    } else {
        *err = "unknown debug tap";
        return -1;
    }
    return n;
}

}  // namespace kns
