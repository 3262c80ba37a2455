// kns_resample.hip -- the sample-rate stages of batch handles that are not at 16 kHz (third extension; section 6).
// resample_kernel<U, D>: the stage "up U, down D", out[U q + p] = sum_j h[r_p + U j] a[D q + e_p - j] with D p = U e_p + r_p -- one
// fmaf per tap from acc = 0, taps ascending, then the synthesis kernel's rounding to int16.  (R, 1) is the interpolator of 8 kHz handles
// and of the out-stages at 32 and 48 kHz, (1, R) the decimator on their other side, (4, 3) (3, 4) and (2, 3) (3, 2) the two stages at 12 and
// 24 kHz.  Plain HIP C++, vector loads and stores only.
//
// One workgroup serves 256 groups q (D input, U output samples each: one to four 16 ms blocks) of ONE stream, a lane one group:
// its U chains share every LDS read, so the phase D n mod U is a compile-time constant of each fmaf.  The group's input and the `hist`
// samples in front of it are staged in LDS as floats, de-interleaved by phase mod D, so that the lanes of a wave read consecutive words
// for every tap; the samples in front of the call come from the stream's state.  The state is a ping-pong pair like the engine's
// history: the row's first workgroup reads the current copy, its last one writes the other (the call's last `hist` input samples), once
// per call.  The taps are wave-uniform: they arrive in the kernel's argument segment, the tap loop is fully unrolled straight-line code,
// so each tap is a scalar load used once.  The tap loop holds no vector-memory operation; the staging loads are unconditional (a clamped
// or selected address); the outputs are assembled in LDS and leave as lane-consecutive stores, guarded once per wave (a frame's outputs
// are a multiple of 64 samples).
//
// Per-frame stream resets (kResets): a stage's history is shorter than a block, so a wave needs its own block's flag only -- where it
// is set, every staged sample in front of the block's first enters its fmaf as +0.
#include "kns_kernels.h"

namespace kns {

namespace {

constexpr int kChunk = 256;  // groups per workgroup
constexpr int kNoFloor = -0x40000000;

__device__ __forceinline__ int16_t to_pcm(float a) {
    a = __builtin_fminf(__builtin_fmaxf(__builtin_roundf(a), -32768.0f), 32767.0f);
    return (int16_t) (int) a;
}

// the row's samples [g0 - hist, g0 - hist + count) as floats, element i through put(i, value); samples in front of the row come from
// `state`, indices behind the row's end (a last, half-filled workgroup's) are clamped onto its last sample and never reach a stored output
template <class Put>
__device__ __forceinline__ void stage(const int16_t *row, const int16_t *state, int hist, int g0, int count, int n_row, Put put) {
    for (int i = threadIdx.x; i < count; i += 256) {
        const int gi = g0 - hist + i;
        const int16_t *p = gi < 0 ? state + i : row + min(gi, n_row - 1);
        put(i, (float) *p);
    }
}

}  // namespace

template <int U, int D, bool kResets>
__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs g) {
    constexpr int K = U > D ? U : D, L = 2 * kRsHalf * K + 1, H = (L - 1) / U;
    constexpr int E = D * (U - 1) / U;             // the newest input a group's outputs read is a[D q + E]
    constexpr int W = (H + kChunk * D + D - 1) / D;  // words per input phase
    __shared__ float xs[D * W];                    // sample m (counted from the first history sample) at [m % D][m / D]
    __shared__ int16_t ys[kChunk * U];
    const int NQ = g.T * g.q_frame, n_in = NQ * D, n_out = NQ * U, chunks = (NQ + kChunk - 1) / kChunk;
    const int b = blockIdx.x / chunks, q0 = (blockIdx.x - b * chunks) * kChunk, n = threadIdx.x, gq = q0 + n;
    const int16_t *row = g.in + (size_t) b * n_in;
    int16_t *orow = g.out + (size_t) b * n_out;
    stage(row, g.state + (size_t) b * H, H, q0 * D, H + kChunk * D, n_in, [&](int i, float v) { xs[(i % D) * W + i / D] = v; });
    if (q0 + kChunk >= NQ && n < H) g.state_next[(size_t) b * H + n] = row[n_in - H + n];  // (a call has more than H input samples)
    __syncthreads();
    int floor_ = kNoFloor;
    if (kResets) {
        const int t = min(gq, NQ - 1) / g.q_frame;
        floor_ = g.resets[(size_t) b * g.T + t] ? t * g.q_frame * D : kNoFloor;
    }
    float acc[U];
#pragma unroll
    for (int p = 0; p < U; ++p) acc[p] = 0.0f;
#pragma unroll
    for (int d = 0; d <= E + H; ++d) {
        // input D gq + E - d = staged sample D n + (H + E - d): phase (H + E - d) mod D, word n + (H + E - d) / D
        float x = xs[((H + E - d) % D) * W + (H + E - d) / D + n];
        if (kResets) x = gq * D + E - d >= floor_ ? x : 0.0f;
#pragma unroll
        for (int p = 0; p < U; ++p) {
            const int j = d - (E - D * p / U), i = D * p % U + U * j;  // chain p: tap r_p + U j on a[D q + e_p - j]
            if (j >= 0 && i < L) acc[p] = fmaf(g.taps[i], x, acc[p]);
        }
    }
#pragma unroll
    for (int p = 0; p < U; ++p) ys[n * U + p] = to_pcm(acc[p]);
    __syncthreads();
#pragma unroll
    for (int k = n; k < kChunk * U; k += 256) {
        if (q0 * U + k < n_out) orow[(size_t) q0 * U + k] = ys[k];  // (wave-uniform: a frame's outputs are a multiple of 64)
    }
}

__global__ __launch_bounds__(256) void resample_reset_kernel(int16_t *state0, int16_t *state1, int hist, const uint8_t *mask, int Bpad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Bpad * hist) return;
    if (!mask || mask[i / hist]) state0[i] = 0, state1[i] = 0;
}

// one workgroup per stream; a listed stream's rs_in and rs_out move as int16, the record's padding is written as zeros
__global__ __launch_bounds__(256) void resample_state_kernel(ResampleStateArgs g) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int rec = g.rec_of[b];
    if (rec < 0) return;
    int16_t *r = (int16_t *) (g.records + (size_t) rec * g.rec_bytes);
    const int n = g.hist_in + g.hist_out, words = (int) (g.rec_bytes / 2);
    if (tid >= words) return;
    const size_t off = tid < g.hist_in ? (size_t) b * g.hist_in + tid : (size_t) b * g.hist_out + (tid - g.hist_in);
    int16_t *const *s = tid < g.hist_in ? g.state_in : g.state_out;
    if (g.import) {
        if (tid < n) s[0][off] = r[tid], s[1][off] = r[tid];
    } else {
        r[tid] = tid < n ? s[0][off] : (int16_t) 0;
    }
}

void launch_resample(const ResampleArgs &a, hipStream_t s) {
    const dim3 grid((unsigned) a.B * (unsigned) ((a.T * a.q_frame + kChunk - 1) / kChunk)), block(256);
#define KNS_RS(UU, DD)                                                                                  \
    do {                                                                                                \
        if (a.resets) hipLaunchKernelGGL((resample_kernel<UU, DD, true>), grid, block, 0, s, a); \
        else hipLaunchKernelGGL((resample_kernel<UU, DD, false>), grid, block, 0, s, a);         \
    } while (0)
    switch (a.U * 8 + a.D) {
        case 2 * 8 + 1: KNS_RS(2, 1); break;  // 8 kHz in; 32 kHz out
        case 3 * 8 + 1: KNS_RS(3, 1); break;  // 48 kHz out
        case 1 * 8 + 2: KNS_RS(1, 2); break;  // 32 kHz in; 8 kHz out
        case 1 * 8 + 3: KNS_RS(1, 3); break;  // 48 kHz in
        case 2 * 8 + 3: KNS_RS(2, 3); break;  // 24 kHz in
        case 3 * 8 + 2: KNS_RS(3, 2); break;  // 24 kHz out
        case 4 * 8 + 3: KNS_RS(4, 3); break;  // 12 kHz in
        default: KNS_RS(3, 4); break;         // 12 kHz out
    }
#undef KNS_RS
}

void launch_resample_reset(int16_t *state0, int16_t *state1, int hist, const uint8_t *mask, int Bpad, hipStream_t s) {
    hipLaunchKernelGGL(resample_reset_kernel, dim3((Bpad * hist + 255) / 256), dim3(256), 0, s, state0, state1, hist, mask, Bpad);
}

void launch_resample_state(const ResampleStateArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(resample_state_kernel, dim3(a.Bpad), dim3(256), 0, s, a);
}

}  // namespace kns
