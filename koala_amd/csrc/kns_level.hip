// kns_level.hip -- output leveller (eleventh extension; section 6): a per-stream, speech-gated automatic gain on the
// samples E of the 16 kHz call, directly behind it, so every rate, sample format, channel layout and packet handle gets it.  Two launches:
//
// level_track_kernel: one lane per stream, sequential over the call's T report rows (e_out, mask_sum).  A frame the network passed
//   (mask_sum / 257 >= theta) and that is above the floor (e_out > e_floor) moves the stream's tracked speech energy lvl, one-pole, up with
//   a_up and down with a_down; the gain the level asks for, sqrt(target / lvl) clamped to [max_cut, max_boost], is approached with slew:
//       speech  = mask_sum * (1/257) >= theta  and  e_out > e_floor
//       lvl     = e_out if lvl == 0 else lvl + a * (e_out - lvl)          (speech frames only; a = a_up if e_out > lvl else a_down)
//       want    = 1 if lvl == 0 else min(max_boost, max(max_cut, sqrt(target / lvl)))
//       g_t     = gain + slew * (want - gain);  gain = g_t
//   Every operation is one fp32 operation, none contracted; the division and the square root are the correctly rounded ones.  The
//   kernel writes the pair (g_{t-1}, g_t) of every frame to a scratch [B][T][2] -- (1, 1) for a stream that is off or held -- and g_t into
//   column 3 of the caller's report.  A per-frame reset makes a levelling stream's state fresh (lvl = 0, gain = 1) before its frame.
// level_apply_kernel: out[256 t + n] = to_pcm(E[256 t + n] * fmaf(n / 256, g_t - g_{t-1}, g_{t-1})), in place.  32 lanes per frame, eight
//   samples (one 16-byte word) per lane, eight frames per workgroup; rows that are not 16-byte aligned move sample by sample,
//   lane-consecutive.  A frame whose two gains are both exactly 1 is not touched: off and held streams cost no memory traffic.
// Saturation in to_pcm is all that bounds the product here; a stream that needs a ceiling below the rails, or a levelled one that must not
// clip, turns the peak limiter on (kns_limit.hip), whose one launch then takes level_apply_kernel's place.  Precision-blind: int16 samples and the float report only.  Plain HIP C++, vector loads and
// stores only.
#include "kns_kernels.h"

namespace kns {

namespace {

__device__ __forceinline__ int16_t to_pcm(float a) {
    a = __builtin_fminf(__builtin_fmaxf(__builtin_roundf(a), -32768.0f), 32767.0f);
    return (int16_t) (int) a;
}

}  // namespace

__global__ __launch_bounds__(256) void level_track_kernel(LevelArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const LevelSetting s = a.set[b];
    const uint8_t *ctl = a.ctl ? a.ctl + (size_t) b * (a.T + 1) : nullptr;
    float2 *g = (float2 *) a.gains + (size_t) b * a.T;
    if (!s.on || (ctl && ctl[0])) {  // off, or held: the state stays, the samples stay
        for (int t = 0; t < a.T; ++t) g[t] = make_float2(1.0f, 1.0f);
        return;
    }
    float lvl = a.state[2 * b], gain = a.state[2 * b + 1];
    for (int t = 0; t < a.T; ++t) {
        if (ctl && ctl[1 + t]) lvl = 0.0f, gain = 1.0f;
        const float *row = a.report + ((size_t) b * a.T + t) * 4;
        const float e = row[1], m = row[2] * (1.0f / 257.0f);
        if (m >= s.theta && e > s.e_floor) {
            if (lvl == 0.0f) {
                lvl = e;
            } else {
                const float d = e - lvl, p = (e > lvl ? s.a_up : s.a_down) * d;
                lvl = lvl + p;
            }
        }
        float want = 1.0f;
        if (lvl != 0.0f) want = __builtin_fminf(s.max_boost, __builtin_fmaxf(s.max_cut, __builtin_sqrtf(s.target / lvl)));
        const float d = want - gain, p = s.slew * d, gt = gain + p;
        g[t] = make_float2(gain, gt);
        if (a.report_out) a.report_out[((size_t) b * a.T + t) * 4 + 3] = gt;
        gain = gt;
    }
    a.state[2 * b] = lvl, a.state[2 * b + 1] = gain;
}

__global__ __launch_bounds__(256) void level_apply_kernel(const float *gains, int16_t *out, int frames, int aligned) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;  // frame b T + t of the call, lane of the frame
    if (f >= frames) return;
    const float2 g = ((const float2 *) gains)[f];
    if (g.x == 1.0f && g.y == 1.0f) return;
    const float d = g.y - g.x;
    int16_t *row = out + (size_t) f * kFrame;
    if (aligned) {
        union {
            uint4 w;
            int16_t v[8];
        } u;
        u.w = ((const uint4 *) row)[l];
#pragma unroll
        for (int k = 0; k < 8; ++k) u.v[k] = to_pcm((float) u.v[k] * fmaf((float) (8 * l + k) * (1.0f / 256.0f), d, g.x));
        ((uint4 *) row)[l] = u.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int n = 32 * k + l;
            row[n] = to_pcm((float) row[n] * fmaf((float) n * (1.0f / 256.0f), d, g.x));
        }
    }
}

// the state of the streams with mask[b] != 0 (null: all) := fresh
__global__ __launch_bounds__(256) void level_reset_kernel(float *state, const uint8_t *mask, int Bpad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= Bpad || (mask && !mask[b])) return;
    state[2 * b] = 0.0f, state[2 * b + 1] = 1.0f;
}

void launch_level(const LevelArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(level_track_kernel, dim3((a.B + 255) / 256), dim3(256), 0, s, a);
    const int frames = a.B * a.T;
    hipLaunchKernelGGL(level_apply_kernel, dim3((frames + 7) / 8), dim3(256), 0, s, a.gains, a.out, frames, ((uintptr_t) a.out & 15) == 0 ? 1 : 0);
}

void launch_level_track(const LevelArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(level_track_kernel, dim3((a.B + 255) / 256), dim3(256), 0, s, a);
}

void launch_level_reset(float *state, const uint8_t *mask, int Bpad, hipStream_t s) {
    hipLaunchKernelGGL(level_reset_kernel, dim3((Bpad + 255) / 256), dim3(256), 0, s, state, mask, Bpad);
}

}  // namespace kns
