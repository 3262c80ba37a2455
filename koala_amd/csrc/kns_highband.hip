// kns_highband.hip -- high-band carry of frame handles at 32 and 48 kHz (ninth extension; section 6).  Both sample-rate
// stages of such a handle are the same low-pass, so what the handle delivers, E, holds nothing above the stages' pass band.  This kernel
// adds the band the 16 kHz call never saw: hb[n] = x[n - D] - Lf[n], where D is the handle's delay and Lf is the out-stage's sum (float, not
// rounded) over the in-stage's output delayed by one engine frame -- the handle with the engine replaced by a pure delay -- scaled by a
// broadband gain G[n] that ramps between the per-frame values s' = g + (1 - g) mask_sum / 257 of the call's own report, the overlap-add's
// cross-fade: out[n] = to_pcm(fmaf(G[n], hb[n], (float) E[n])).  Precision-blind: it sees int16 samples and the float report only.
// Plain HIP C++, vector loads and stores only.
//
// high_band_kernel<R>: the work split of resample_kernel<R, 1>.  A workgroup is the 256 groups q of ONE frame of ONE stream, a lane one q and
// its R outputs.  The delayed in-stage output is staged in LDS as floats (304 of them: lane n reads words n + 48 - d, consecutive over the
// lanes for every tap d); the taps are wave-uniform, read from the argument segment by the fully unrolled tap loop, which holds no
// vector-memory operation; x, E and out move lane-consecutive and are assembled in LDS; E is read and out is written in place.  The gains are
// wave-uniform too: three report rows (times the channels of a linked group) per workgroup.  The staging loads are unconditional (a selected
// address).  The state is a ping-pong pair: every workgroup of a row may read the current copy (D is longer than a frame), its last one
// writes the other, once per call.
//
// Not yet: 24 kHz and 44.1 / 22.05 kHz; packet handles; stream records of this state; held streams; per-frame resets behind frame 0 (a
// frame-0 flag makes everything in front of the call read as zero); any change to the low band, the model or the mask.
#include "kns_kernels.h"

namespace kns {

namespace {

__device__ __forceinline__ int16_t to_pcm(float a) {
    a = __builtin_fminf(__builtin_fmaxf(__builtin_roundf(a), -32768.0f), 32767.0f);
    return (int16_t) (int) a;
}

// the attenuation limit's own two roundings (kns_stft.hip, min_gain_mask), u = 1 - g
__device__ __forceinline__ float limited(float g, float u, float m) {
#pragma clang fp contract(off)
    const float p = u * m;
    return g + p;
}

}  // namespace

template <int R>
__global__ __launch_bounds__(256) void high_band_kernel(HighBandArgs g) {
    constexpr int H = 2 * kRsHalf, L = H * R + 1, XH = hb_x_hist(R), F = kFrame * R;
    __shared__ float yd[kHbYHist];  // y[256 t - 304 + i]: the delayed in-stage output the frame's chains read
    __shared__ int16_t xd[F];       // x[R (256 t - 304) + k] = x[n - D] of the frame's outputs
    __shared__ int16_t es[F];       // E, then out
    const int b = blockIdx.x / g.T, t = blockIdx.x - b * g.T, n = threadIdx.x, q0 = t * kFrame;
    const bool fresh = g.resets && g.resets[(size_t) b * g.T] != 0;
    const int16_t *xrow = g.x + (size_t) b * g.T * F, *yrow = g.y + (size_t) b * g.T * kFrame;
    int16_t *orow = g.out + (size_t) b * g.T * F + (size_t) t * F;
    const int16_t *xs = g.xs + (size_t) b * XH, *ys = g.ys + (size_t) b * kHbYHist;
    // samples in front of the call come from the state (a fresh stream: zeros); every index lies inside its row or its state
    for (int i = n; i < kHbYHist; i += 256) {
        const int gi = q0 - kHbYHist + i;
        const float v = (float) *(gi < 0 ? ys + (kHbYHist + gi) : yrow + gi);
        yd[i] = gi < 0 && fresh ? 0.0f : v;
    }
#pragma unroll
    for (int k = n; k < F; k += 256) {
        const int gi = R * (q0 - kHbYHist) + k;
        const int16_t v = *(gi < 0 ? xs + (XH + gi) : xrow + gi);
        xd[k] = gi < 0 && fresh ? (int16_t) 0 : v;
        es[k] = orow[k];
    }
    // the broadband gains of frames t, t - 1 and t - 2 (wave-uniform)
    const int C = g.link > 1 ? g.link : 1, b0 = b - b % C;
    const float mg = g.min_gain ? g.min_gain[b] : 0.0f, mu = 1.0f - mg;
    float sp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int tt = t - k;
        if (tt < 0) {
            sp[k] = fresh ? 0.0f : g.ss[(size_t) b * 2 + (-1 - tt)];
        } else {
            float s = 0.0f;
            for (int c = 0; c < C; ++c) s = __builtin_fmaxf(s, g.report[((size_t) (b0 + c) * g.T + tt) * 4 + 2] * (1.0f / 257.0f));
            sp[k] = limited(mg, mu, s);
        }
    }
    if (t == g.T - 1) {  // the row's last workgroup: the state behind the call
        int16_t *xn = g.xs_next + (size_t) b * XH, *yn = g.ys_next + (size_t) b * kHbYHist;
        for (int i = n; i < kHbYHist; i += 256) {
            const int gi = g.T * kFrame - kHbYHist + i;
            const int16_t v = *(gi < 0 ? ys + (kHbYHist + gi) : yrow + gi);
            yn[i] = gi < 0 && fresh ? (int16_t) 0 : v;
        }
        for (int i = n; i < XH; i += 256) {
            const int gi = g.T * F - XH + i;
            const int16_t v = *(gi < 0 ? xs + (XH + gi) : xrow + gi);
            xn[i] = gi < 0 && fresh ? (int16_t) 0 : v;
        }
        if (n < 2) g.ss_next[(size_t) b * 2 + n] = n ? sp[1] : sp[0];
    }
    __syncthreads();
    // G: output group q belongs to the engine's sample j = q - 24 (the out-stage's delay): the lanes in front of 24 still ramp in frame t - 1
    const bool early = n < kRsHalf;
    const float hi = early ? sp[1] : sp[0], lo = early ? sp[2] : sp[1];
    const float w = (float) (early ? n + kFrame - kRsHalf : n - kRsHalf) * (1.0f / 256.0f);
    const float G = fmaf(w, hi - lo, lo);
    float acc[R];
#pragma unroll
    for (int p = 0; p < R; ++p) acc[p] = 0.0f;
#pragma unroll
    for (int d = 0; d <= H; ++d) {  // the out-stage's chains over yd[q - d]: tap p + R d, ascending
        const float v = yd[n + H - d];
#pragma unroll
        for (int p = 0; p < R; ++p)
            if (p + R * d < L) acc[p] = fmaf(g.taps[p + R * d], v, acc[p]);
    }
#pragma unroll
    for (int p = 0; p < R; ++p) {
        const float hb = (float) xd[n * R + p] - acc[p];
        es[n * R + p] = to_pcm(fmaf(G, hb, (float) es[n * R + p]));
    }
    __syncthreads();
#pragma unroll
    for (int k = n; k < F; k += 256) orow[k] = es[k];
}

__global__ __launch_bounds__(256) void high_band_reset_kernel(int16_t *x0, int16_t *x1, int16_t *y0, int16_t *y1, float *s0, float *s1, int xh,
                                                              const uint8_t *mask, int Bpad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Bpad * xh) return;
    const int b = i / xh, k = i - b * xh;
    if (mask && !mask[b]) return;
    x0[i] = 0, x1[i] = 0;
    if (k < kHbYHist) y0[b * kHbYHist + k] = 0, y1[b * kHbYHist + k] = 0;
    if (k < 2) s0[b * 2 + k] = 0.0f, s1[b * 2 + k] = 0.0f;
}

void launch_high_band(const HighBandArgs &a, hipStream_t s) {
    const dim3 grid((unsigned) a.B * (unsigned) a.T), block(256);
    if (a.R == 2) hipLaunchKernelGGL(high_band_kernel<2>, grid, block, 0, s, a);  // 32 kHz
    else hipLaunchKernelGGL(high_band_kernel<3>, grid, block, 0, s, a);          // 48 kHz
}

void launch_high_band_reset(int16_t *const xs[2], int16_t *const ys[2], float *const ss[2], int R, const uint8_t *mask, int Bpad, hipStream_t s) {
    const int xh = hb_x_hist(R);
    hipLaunchKernelGGL(high_band_reset_kernel, dim3((Bpad * xh + 255) / 256), dim3(256), 0, s, xs[0], xs[1], ys[0], ys[1], ss[0], ss[1], xh, mask, Bpad);
}

}  // namespace kns
