// kns_fractional.hip -- the fractional sample-rate stages of packet handles at 44 100 and 22 050 Hz (sixth extension;
// section 6).  16 000 / rate is U / 441 with U = 160 or 320, so the stages are "up U, down 441" in front of the 16 kHz packet path and
// "up 441, down U" behind it, over the prototype of K = 441: 21 169 taps, of which one output sees at most 133 / 67 (in) or 49 (out).
// Plain HIP C++, vector loads and stores only.
//
// resample_kernel<U, D> (kns_resample.hip) cannot serve: there a lane owns a whole group of D inputs and U outputs and every tap is a scalar
// operand.  Here a lane owns ONE output; consecutive outputs advance the phase by 441 mod U (in) or U mod 441 (out), so the lanes of a wave
// sit at different phases and read their taps themselves, from the polyphase table [tap j][phase r] in global memory: at a fixed j the
// lanes of a wave read inside one row of U or 441 floats, a handful of cache lines that every workgroup of every call reads again.
//
// One workgroup serves ONE stream, as the packet kernels do: the counts come from the call's device table, the per-stream time base
// N mod 441 from the stage's own copy of it.  The stream's history goes to LDS first, so it is rewritten in place behind the last chunk
// (no other workgroup reads it); the outputs are produced in chunks of 256, a chunk's input span -- history included -- staged in LDS as
// floats.  The tap loop holds one table load, one LDS read and one fmaf per tap, ascending, from acc = 0; then the synthesis kernel's
// rounding to int16.  A tap that does not exist (r + P j >= L) is a zero of the table on a staged finite sample: the chain's value stays.
// counts[b] == 0 touches nothing.  Every index is bounded by the stream's count and phase: a lane past the stream's last output computes
// that last output again and stores nothing.
#include "kns_kernels.h"

namespace kns {

namespace {

constexpr int kFrChunk = 256;  // outputs per chunk: one per lane

__device__ __forceinline__ int16_t fr_to_pcm(float a) {
    a = __builtin_fminf(__builtin_fmaxf(__builtin_roundf(a), -32768.0f), 32767.0f);
    return (int16_t) (int) a;
}

// the last H of [old (H samples) | row (n samples)] -> hist, in place: `old` is the LDS copy
template <int H>
__device__ __forceinline__ void fr_keep(int16_t *hist, const int16_t *old, const int16_t *row, int n) {
    for (int i = threadIdx.x; i < H; i += 256) hist[i] = n + i < H ? old[n + i] : row[n + i - H];
}

}  // namespace

// y[m] = sum over i = 441 m mod U, + U, ... < L of h[i] x[(441 m - i) / U], for the inner samples m in [M(N), M(N + count))
template <int U>
__global__ __launch_bounds__(256) void fractional_in_kernel(FractionalArgs g) {
    constexpr int T = fr_in_taps(U);                                   // taps of an output = samples kept per stream
    constexpr int W = T + (kFrChunk - 1) * kFrDown / U + 2;            // a chunk's input span: its first output's taps, then ~441 / U per output
    __shared__ int16_t old[T];
    __shared__ float xs[W];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ph = g.phase[b], count = g.counts[b];
    if (count == 0) return;
    const int m0 = (int) fr_inner(ph, U), m = (int) fr_inner(ph + count, U) - m0;
    int16_t *hist = g.hist + (size_t) b * T;
    const int16_t *row = g.in + (size_t) b * g.in_stride;
    int16_t *orow = g.out + (size_t) b * g.out_stride;
    for (int i = tid; i < T; i += 256) old[i] = hist[i];
    __syncthreads();
    // samples are counted from the start of the stream's 441-cycle: the call's first is ph, and an output's newest is 441 m / U >= ph
    for (int o0 = 0; o0 < m; o0 += kFrChunk) {
        const int base = kFrDown * (m0 + o0) / U - (T - 1);  // >= ph - (T - 1): inside the history
        for (int i = tid; i < W; i += 256) {
            const int c = base + i - ph;
            xs[i] = (float) (c < 0 ? old[T + c] : row[min(c, count - 1)]);
        }
        __syncthreads();
        const int t = kFrDown * (m0 + min(o0 + tid, m - 1)), e = t / U;
        const float *tap = g.taps + (t - U * e);
        const float *x = xs + (e - base);
        float acc = 0.0f;
#pragma unroll 7
        for (int j = 0; j < T; ++j) acc = fmaf(tap[j * U], x[-j], acc);
        if (o0 + tid < m) orow[o0 + tid] = fr_to_pcm(acc);
        __syncthreads();
    }
    fr_keep<T>(hist, old, row, count);
    if (tid == 0) g.phase[b] = (ph + count) % kFrDown;
}

// z[n] = sum over i = p mod 441, + 441, ... < L of h[i] v[(p - i) / 441], p = U n - c, for the outputs n in [N, N + count)
template <int U>
__global__ __launch_bounds__(256) void fractional_out_kernel(FractionalArgs g) {
    constexpr int T = kFrOutTaps, H = kFrOutHist, C = fr_shift(U);
    constexpr int W = T + (kFrChunk - 1) * U / kFrDown + 3;
    __shared__ int16_t old[H];
    __shared__ float xs[W];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ph = g.phase[b], count = g.counts[b];
    if (count == 0) return;
    const int m0 = (int) fr_inner(ph, U), m = (int) fr_inner(ph + count, U) - m0;  // the call's inner samples: row[0 .. m)
    int16_t *hist = g.hist + (size_t) b * H;
    const int16_t *row = g.in + (size_t) b * g.in_stride;
    int16_t *orow = g.out + (size_t) b * g.out_stride;
    for (int i = tid; i < H; i += 256) old[i] = hist[i];
    __syncthreads();
    // inner samples are counted from the start of the stream's cycle: the call's first is m0.  p >= -c > -441: floor(p / 441) = (p + 441) / 441 - 1
    for (int o0 = 0; o0 < count; o0 += kFrChunk) {
        const int base = (U * (ph + o0) - C + kFrDown) / kFrDown - 1 - (T - 1);
        for (int i = tid; i < W; i += 256) {
            const int w = base + i - m0;  // (an existing tap reads w in [-H, m); the rest is bounds only)
            xs[i] = (w < -H || (m == 0 && w >= 0)) ? 0.0f : (float) (w < 0 ? old[H + w] : row[min(w, m - 1)]);
        }
        __syncthreads();
        const int p = U * (ph + min(o0 + tid, count - 1)) - C, e = (p + kFrDown) / kFrDown - 1;
        const float *tap = g.taps + (p - kFrDown * e);
        const float *x = xs + (e - base);
        float acc = 0.0f;
#pragma unroll 7
        for (int j = 0; j < T; ++j) acc = fmaf(tap[j * kFrDown], x[-j], acc);
        if (o0 + tid < count) orow[o0 + tid] = fr_to_pcm(acc);
        __syncthreads();
    }
    fr_keep<H>(hist, old, row, m);
    if (tid == 0) g.phase[b] = (ph + count) % kFrDown;
}

// the streams with mask[b] != 0 (null: all): both histories zeros, N mod 441 = 0
__global__ __launch_bounds__(256) void fractional_reset_kernel(FractionalStateArgs g, const uint8_t *mask) {
    const int i = blockIdx.x * 256 + threadIdx.x, row = g.taps_in + kFrOutHist;
    if (i >= g.Bpad * row) return;
    const int b = i / row, k = i - b * row;
    if (mask && !mask[b]) return;
    if (k < g.taps_in) g.hist_in[(size_t) b * g.taps_in + k] = 0;
    else g.hist_out[(size_t) b * kFrOutHist + (k - g.taps_in)] = 0;
    if (k == 0) g.phase_in[b] = 0, g.phase_out[b] = 0;
}

void launch_fractional_in(const FractionalArgs &a, int B, hipStream_t s) {
    if (a.U == 160) hipLaunchKernelGGL(fractional_in_kernel<160>, dim3(B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(fractional_in_kernel<320>, dim3(B), dim3(256), 0, s, a);
}

void launch_fractional_out(const FractionalArgs &a, int B, hipStream_t s) {
    if (a.U == 160) hipLaunchKernelGGL(fractional_out_kernel<160>, dim3(B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(fractional_out_kernel<320>, dim3(B), dim3(256), 0, s, a);
}

void launch_fractional_reset(const FractionalStateArgs &a, const uint8_t *mask, hipStream_t s) {
    hipLaunchKernelGGL(fractional_reset_kernel, dim3((a.Bpad * (a.taps_in + kFrOutHist) + 255) / 256), dim3(256), 0, s, a, mask);
}

}  // namespace kns
