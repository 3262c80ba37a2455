// kns_packet.hip -- the packetiser of packet handles (fourth extension; section 6): streams that take and deliver any
// number of samples per call around the unchanged frame call.  Plain HIP C++, vector loads and stores only.
//
// packet_in_kernel:  per stream, [pending input | the call's samples] -> the whole frames of the call's sub-calls (dense [B][T F] matrices,
//                    stacked one behind the other) and the new pending input; the rows of sub-calls that hold the stream are zeros.
// packet_out_kernel: per stream, [pending output | the enhanced frames of its sub-calls] -> the caller's row and the new pending output;
//                    with a report, the stream's rows of the sub-calls' reports -> report[b][0 .. k_b).
//
// One workgroup serves one stream: a stream's call is a copy of a few hundred samples whose source and destination differ by an
// arbitrary (odd as often as even) sample offset.  The old pending samples go to LDS first, so the pending buffers are rewritten in place;
// every destination row is then produced in segments staged through LDS at the DESTINATION's 16-byte phase: the source is read sample by
// sample (consecutive lanes, consecutive samples), the destination is written as aligned 16-byte words, with single samples only at a
// row's two ragged ends.  Every index is bounded by the stream's count, fill and frame count, which the host has checked.
#include "kns_kernels.h"

namespace kns {

namespace {

constexpr int kSeg = 2048;        // samples per staged segment
constexpr int kMaxFrame = 768;    // the longest frame (48 kHz)

// the sub-call that holds frame f of the call: cut[l] <= f < cut[l + 1] (a call has a handful of sub-calls)
__device__ __forceinline__ int sub_of(const int32_t *cut, int nsub, int f) {
    int l = 0;
    while (l + 1 < nsub && f >= cut[l + 1]) ++l;
    return l;
}

// dst[0 .. n) = src(0 .. n), n uniform over the workgroup; `seg` holds kSeg + 8 samples, 16-byte aligned
template <class Src>
__device__ __forceinline__ void put_row(int16_t *dst, int n, int16_t *seg, Src src) {
    if (n <= 0) return;
    const int tid = threadIdx.x;
    const int a = (int) (((uintptr_t) dst >> 1) & 7);  // dst - a is 16-byte aligned: sample i of the row is word-position v = a + i
    int16_t *base = dst - a;                           // (never dereferenced below position a)
    for (int v0 = 0; v0 < a + n; v0 += kSeg) {
        const int v1 = min(v0 + kSeg, a + n);
        for (int v = v0 + tid; v < v1; v += 256)
            if (v >= a) seg[v - v0] = src(v - a);
        __syncthreads();
        for (int g = v0 + 8 * tid; g < v1; g += 8 * 256) {
            if (g >= a && g + 8 <= a + n) {
                *(uint4 *) (base + g) = *(const uint4 *) (seg + (g - v0));
            } else {
                for (int j = 0; j < 8; ++j)
                    if (g + j >= a && g + j < a + n) base[g + j] = seg[g + j - v0];
            }
        }
        __syncthreads();
    }
}

}  // namespace

__global__ __launch_bounds__(256) void packet_in_kernel(PacketArgs g) {
    __shared__ int16_t old[kMaxFrame];
    __shared__ __attribute__((aligned(16))) int16_t seg[kSeg + 8];
    const int b = blockIdx.x, tid = threadIdx.x, F = g.F;
    const int fill = g.fill_in[b], count = g.tab[b];
    const int total = fill + count, k = total / F, new_fill = total - k * F;
    const int nsub = g.tab[g.Bpad];
    const int32_t *cut = g.tab + g.Bpad + 1;
    int16_t *pin = g.pin + (size_t) b * F;
    const int16_t *row = g.user_in + (size_t) b * g.max_samples;
    for (int i = tid; i < fill; i += 256) old[i] = pin[i];
    __syncthreads();
    for (int l = 0; l < nsub; ++l) {
        const int c0 = cut[l], T = cut[l + 1] - c0, n = T * F;
        int16_t *dst = g.frames + (size_t) g.B * F * c0 + (size_t) b * n;  // (a multiple of 256 bytes from the allocation's start)
        if (k > c0) {  // (the plan cuts at every stream's frame count: k >= cut[l + 1] then)
            const int s0 = c0 * F;
            put_row(dst, n, seg, [&](int i) { const int c = s0 + i; return c < fill ? old[c] : row[c - fill]; });
        } else {  // held in this sub-call: the inner call reads the row
            for (int i = 8 * tid; i < n; i += 8 * 256) *(uint4 *) (dst + i) = make_uint4(0, 0, 0, 0);
        }
    }
    const int s0 = k * F;
    put_row(pin, new_fill, seg, [&](int i) { const int c = s0 + i; return c < fill ? old[c] : row[c - fill]; });
    if (tid == 0) g.fill_in[b] = new_fill;
}

__global__ __launch_bounds__(256) void packet_out_kernel(PacketArgs g) {
    __shared__ int16_t old[kMaxFrame];
    __shared__ __attribute__((aligned(16))) int16_t seg[kSeg + 8];
    const int b = blockIdx.x, tid = threadIdx.x, F = g.F;
    const int fill = g.fill_out[b], count = g.tab[b], P = F - 1 - fill;  // P pending output samples
    const int total = fill + count, k = total / F, new_fill = total - k * F;
    const int nsub = g.tab[g.Bpad];
    const int32_t *cut = g.tab + g.Bpad + 1;
    int16_t *pout = g.pout + (size_t) b * F;
    for (int i = tid; i < P; i += 256) old[i] = pout[i];
    __syncthreads();
    // sample c of [pending output | enhanced frames]: c < P + k F
    auto src = [&](int c) -> int16_t {
        if (c < P) return old[c];
        const int j = c - P, f = j / F, l = sub_of(cut, nsub, f), c0 = cut[l], T = cut[l + 1] - c0;
        return g.frames[(size_t) g.B * F * c0 + ((size_t) b * T + (f - c0)) * F + (j - f * F)];
    };
    put_row(g.user_out + (size_t) b * g.max_samples, count, seg, src);
    put_row(pout, F - 1 - new_fill, seg, [&](int i) { return src(count + i); });
    if (tid == 0) g.fill_out[b] = new_fill;
    if (g.report) {
        for (int i = tid; i < 4 * k; i += 256) {
            const int f = i >> 2, l = sub_of(cut, nsub, f), c0 = cut[l], T = cut[l + 1] - c0;
            g.report[((size_t) b * g.report_frames + f) * 4 + (i & 3)] =
                g.sub_report[(size_t) g.B * c0 * 4 + ((size_t) b * T + (f - c0)) * 4 + (i & 3)];
        }
    }
}

// the streams with mask[b] != 0 (null: all): fill = 0, pending output = F - 1 zeros
__global__ __launch_bounds__(256) void packet_reset_kernel(PacketStateArgs g, const uint8_t *mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.Bpad * g.F) return;
    const int b = i / g.F;
    if (mask && !mask[b]) return;
    g.pin[i] = 0, g.pout[i] = 0;
    if (i == b * g.F) g.fill_in[b] = 0, g.fill_out[b] = 0;
}

// one workgroup per stream; a listed stream's packet part of its record: uint32 fill, int16[F - 1] = [pending input | pending output],
// zero padding.  (Between calls fill_in == fill_out.)
__global__ __launch_bounds__(256) void packet_state_kernel(PacketStateArgs g) {
    const int b = blockIdx.x, tid = threadIdx.x, F = g.F;
    const int rec = g.rec_of[b];
    if (rec < 0) return;
    uint8_t *r = g.records + (size_t) rec * g.rec_bytes;
    int16_t *buf = (int16_t *) (r + 4);
    int16_t *pin = g.pin + (size_t) b * F, *pout = g.pout + (size_t) b * F;
    const int words = (int) (g.rec_bytes - 4) / 2;
    if (g.import) {
        const int fill = (int) *(const uint32_t *) r;  // (checked by the host: below F)
        for (int i = tid; i < F - 1; i += 256) {
            if (i < fill) pin[i] = buf[i];
            else pout[i - fill] = buf[i];
        }
        if (tid == 0) g.fill_in[b] = fill, g.fill_out[b] = fill;
    } else {
        const int fill = g.fill_in[b];
        for (int i = tid; i < words; i += 256) buf[i] = i >= F - 1 ? (int16_t) 0 : i < fill ? pin[i] : pout[i - fill];
        if (tid == 0) *(uint32_t *) r = (uint32_t) fill;
    }
}

void launch_packet_in(const PacketArgs &a, hipStream_t s) { hipLaunchKernelGGL(packet_in_kernel, dim3(a.B), dim3(256), 0, s, a); }
void launch_packet_out(const PacketArgs &a, hipStream_t s) { hipLaunchKernelGGL(packet_out_kernel, dim3(a.B), dim3(256), 0, s, a); }
void launch_packet_reset(const PacketStateArgs &a, const uint8_t *mask, hipStream_t s) {
    hipLaunchKernelGGL(packet_reset_kernel, dim3((a.Bpad * a.F + 255) / 256), dim3(256), 0, s, a, mask);
}
void launch_packet_state(const PacketStateArgs &a, hipStream_t s) { hipLaunchKernelGGL(packet_state_kernel, dim3(a.Bpad), dim3(256), 0, s, a); }

}  // namespace kns
