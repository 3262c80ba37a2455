// kns_limit.hip -- peak limiter (thirteenth extension; section 6): a per-stream ceiling c on the samples E of the 16 kHz
// call, instant attack, linear release of delta per sample, in the leveller's place -- so every rate, sample format, channel layout and
// packet handle gets it.  One launch applies the leveller's ramp AND the limiter (it must see the product before saturation), instead of
// level_apply_kernel.  Per stream one float of state, g, the gain behind the last sample; fresh: 1.  For frame t, n = 0 .. 255:
//       r[n]   = fmaf(n / 256, g_t - g_{t-1}, g_{t-1})       (the tracker's pair of this frame; (1, 1) when the stream does not level)
//       v[n]   = float(E[256 t + n]) * r[n]
//       q[n]   = 1 if |v[n]| <= c else c / |v[n]|
//       m_0    = q;   m_{j+1}[n] = min(m_j[n], m_j[n - 2^j] + 2^j delta) for n >= 2^j, else m_j[n]        j = 0 .. 7
//       h[n]   = fmaf(float(n + 1), delta, g)                 (g: the state entering this frame)
//       G[n]   = min(1, min(m_8[n], h[n]));   out[256 t + n] = to_pcm(v[n] * G[n]);   g := G[255]
//   Every line is one fp32 operation, none contracted; the division is the correctly rounded one.  m_8 is the lower envelope
//   min_k (q[n - k] + k delta) inside the frame, formed by doubling in an order the rule fixes; h carries the release across the boundary.
// limit_kernel: one wave per stream, four waves per workgroup; the wave walks the call's T frames in order with g in a register, and a
//   lane holds four consecutive samples (one 8-byte word; rows that are not 8-byte aligned move sample by sample).  Levels 0 and 1 of the
//   envelope take the neighbour lane's last samples, levels 2 .. 7 shift whole lanes by 1 .. 32 (wave shuffles).  The next frame's samples
//   and pair are fetched before this frame's arithmetic.  A frame in which no sample is above the ceiling skips the envelope (m_8 is then
//   exactly 1), and one with ramp (1, 1) and g = 1 besides is not stored.  A stream whose limiter is off, or that the call holds, gets
//   exactly what level_apply_kernel does, and its g does not move.  Precision-blind: int16 samples only.  Plain HIP C++, vector loads and
//   stores only.
#include "kns_kernels.h"

namespace kns {

namespace {

__device__ __forceinline__ int16_t to_pcm(float a) {
    a = __builtin_fminf(__builtin_fmaxf(__builtin_roundf(a), -32768.0f), 32767.0f);
    return (int16_t) (int) a;
}

union Quad {
    uint2 w;
    int16_t v[4];
};

__device__ __forceinline__ Quad load_quad(const int16_t *p, int aligned) {
    Quad u;
    if (aligned) {
        u.w = *(const uint2 *) p;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) u.v[k] = p[k];
    }
    return u;
}

__device__ __forceinline__ void store_quad(int16_t *p, const Quad &u, int aligned) {
    if (aligned) {
        *(uint2 *) p = u.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = u.v[k];
    }
}

}  // namespace

__global__ __launch_bounds__(256) void limit_kernel(LimitArgs a, int aligned) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;  // stream, lane: samples 4 l .. 4 l + 3 of every frame
    if (b >= a.B) return;
    const LimiterSetting s = a.set[b];
    const uint8_t *ctl = a.ctl ? a.ctl + (size_t) b * (a.T + 1) : nullptr;
    const bool live = s.on && !(ctl && ctl[0]);  // (off, or held: the leveller's ramp alone; a held stream's pairs are (1, 1))
    const float2 *pairs = a.gains ? (const float2 *) a.gains + (size_t) b * a.T : nullptr;
    int16_t *row = a.out + (size_t) b * a.T * kFrame + 4 * l;
    const float c = s.ceiling, delta = s.release;
    float g = live ? a.state[b] : 1.0f;
    Quad next = load_quad(row, aligned);
    float2 next_pair = pairs ? pairs[0] : make_float2(1.0f, 1.0f);
    for (int t = 0; t < a.T; ++t) {
        const Quad e = next;
        const float2 p = next_pair;
        if (t + 1 < a.T) {
            next = load_quad(row + (size_t) (t + 1) * kFrame, aligned);
            if (pairs) next_pair = pairs[t + 1];
        }
        const bool flat = p.x == 1.0f && p.y == 1.0f;
        if (live && ctl && ctl[1 + t]) g = 1.0f;
        const float d = p.y - p.x;
        float v[4], q[4];
        bool over = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = (float) e.v[k] * fmaf((float) (4 * l + k) * (1.0f / 256.0f), d, p.x);
            const float m = __builtin_fabsf(v[k]);
            q[k] = m <= c ? 1.0f : c / m;
            over = over || !(m <= c);
        }
        Quad o;
        if (!live) {  // level_apply_kernel's frame
            if (flat) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.v[k] = to_pcm(v[k]);
            store_quad(row + (size_t) t * kFrame, o, aligned);
            continue;
        }
        const bool any_over = __any(over) != 0;  // (wave-uniform)
        if (!any_over && flat && g == 1.0f) continue;  // G == 1 throughout and v == E: the samples stay, g stays
        if (any_over) {
            // levels 0 and 1: the shift is inside the lane's four samples but for its first one or two, which take the lane below's last
            float u2 = __shfl_up(q[2], 1), u3 = __shfl_up(q[3], 1);
            {
                const float m0 = l ? __builtin_fminf(q[0], u3 + delta) : q[0];
                const float m1 = __builtin_fminf(q[1], q[0] + delta), m2 = __builtin_fminf(q[2], q[1] + delta), m3 = __builtin_fminf(q[3], q[2] + delta);
                q[0] = m0, q[1] = m1, q[2] = m2, q[3] = m3;
            }
            u2 = __shfl_up(q[2], 1), u3 = __shfl_up(q[3], 1);
            {
                const float step = 2.0f * delta;
                const float m0 = l ? __builtin_fminf(q[0], u2 + step) : q[0], m1 = l ? __builtin_fminf(q[1], u3 + step) : q[1];
                const float m2 = __builtin_fminf(q[2], q[0] + step), m3 = __builtin_fminf(q[3], q[1] + step);
                q[0] = m0, q[1] = m1, q[2] = m2, q[3] = m3;
            }
            // levels 2 .. 7: whole lanes, 1 .. 32 of them
#pragma unroll
            for (int j = 2; j < 8; ++j) {
                const int lanes = 1 << (j - 2);
                const float step = (float) (1 << j) * delta;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float u = __shfl_up(q[k], lanes);
                    if (l >= lanes) q[k] = __builtin_fminf(q[k], u + step);
                }
            }
        }
        float last = 1.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float h = fmaf((float) (4 * l + k + 1), delta, g);
            const float G = __builtin_fminf(1.0f, __builtin_fminf(q[k], h));
            o.v[k] = to_pcm(v[k] * G);
            last = G;
        }
        store_quad(row + (size_t) t * kFrame, o, aligned);
        g = __shfl(last, 63);
    }
    if (live && l == 0) a.state[b] = g;
}

// g of the streams with mask[b] != 0 (null: all) := 1
__global__ __launch_bounds__(256) void limit_reset_kernel(float *state, const uint8_t *mask, int Bpad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= Bpad || (mask && !mask[b])) return;
    state[b] = 1.0f;
}

void launch_limit(const LimitArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(limit_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a, ((uintptr_t) a.out & 7) == 0 ? 1 : 0);
}

void launch_limit_reset(float *state, const uint8_t *mask, int Bpad, hipStream_t s) {
    hipLaunchKernelGGL(limit_reset_kernel, dim3((Bpad + 255) / 256), dim3(256), 0, s, state, mask, Bpad);
}

}  // namespace kns
