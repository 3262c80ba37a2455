// kns_channels.hip -- multi-channel batch handles (seventh extension; section 6): the caller's `pcm` and `enhanced`
// hold the C streams of a group interleaved, [G][n C] elements, and the engine's rows are [B][n] with stream g C + c = channel c of group g.
// Pure byte movement on elements of W = 1, 2 or 4 bytes (one pair of kernels serves all four sample formats), outermost: in front of and
// behind the format stage.  Plain HIP C++, vector loads and stores only.
//
// channels_split_kernel<W>: [G][n C] -> [B][n], every element of every row
// channels_join_kernel<W>:  [B][n] -> [G][n C]; a packet call writes group g's first counts[g C] C elements only
//
// Both are one routine.  A workgroup takes one span of one group: S samples of each channel, S C W <= 8 KiB.  The LDS holds the span's
// INTERLEAVED bytes at the offsets they have behind the last 16-byte boundary in front of them in global memory, so an aligned 16-byte word of
// the caller's row is an aligned 16-byte word of the image: the interleaved side moves every such word that lies wholly inside the span as one
// uint4 and the rest of the span (its head and tail, at most 15 bytes each) per element.  The channels' side does the same with the aligned
// 16-byte words of each channel's row -- a lane gathers (scatters) the 16 / W elements of one word at their stride of C elements in the image
// -- and with each row's head and tail.  No word is touched that is not wholly inside its span, so nothing outside either matrix is read or
// written, whatever the alignment of the pointers and whatever the row length.
//
// Banks: the gather's lanes are 16 C bytes apart in the image, and ds_read_b32 / _u16 / _u8 and every ds_write bank by (a / 4) % 32 per
// 32-lane half: 2 C-way conflicts for C = 2, 4, 8.  One dword of padding behind every 32 dwords of the image moves lane j by j / (8 / C)
// banks: conflict-free for C = 2, 4 and 8, at most 2-way for the others.
#include "kns_kernels.h"

namespace kns {

namespace {

constexpr int kChImage = kChSpanBytes + 16;                            // the span and the bytes in front of it in its first word
constexpr int kChLds = (kChImage + (kChImage >> 7) * 4 + 15) / 16 * 4;  // dwords, padding included

__device__ __forceinline__ int pad(int a) { return a + ((a >> 7) << 2); }

template <int W>
__device__ __forceinline__ uint32_t lds_get(const uint32_t *lds, int a) {
    if (W == 4) return lds[pad(a) >> 2];
    if (W == 2) return ((const uint16_t *) lds)[pad(a) >> 1];
    return ((const uint8_t *) lds)[pad(a)];
}
template <int W>
__device__ __forceinline__ void lds_put(uint32_t *lds, int a, uint32_t bits) {
    if (W == 4) lds[pad(a) >> 2] = bits;
    else if (W == 2) ((uint16_t *) lds)[pad(a) >> 1] = (uint16_t) bits;
    else ((uint8_t *) lds)[pad(a)] = (uint8_t) bits;
}
template <int W>
__device__ __forceinline__ uint32_t load_one(const uint8_t *p) {
    if (W == 4) return *(const uint32_t *) p;
    if (W == 2) return *(const uint16_t *) p;
    return *p;
}
template <int W>
__device__ __forceinline__ void store_one(uint8_t *p, uint32_t bits) {
    if (W == 4) *(uint32_t *) p = bits;
    else if (W == 2) *(uint16_t *) p = (uint16_t) bits;
    else *p = (uint8_t) bits;
}
// element i of a packed 16-byte word of W-byte elements
template <int W>
__device__ __forceinline__ uint32_t get(const uint32_t *x, int i) {
    if (W == 4) return x[i];
    if (W == 2) return (x[i >> 1] >> (16 * (i & 1))) & 0xFFFF;
    return (x[i >> 2] >> (8 * (i & 3))) & 0xFF;
}
template <int W>
__device__ __forceinline__ void put(uint32_t *y, int i, uint32_t bits) {
    if (W == 4) y[i] = bits;
    else if (W == 2) y[i >> 1] |= (bits & 0xFFFF) << (16 * (i & 1));
    else y[i >> 2] |= (bits & 0xFF) << (8 * (i & 3));
}

// The interleaved side of a span: global bytes [I, I + L), image offsets [a, a + L) with a = I mod 16.  ToLds: global -> image, else back.
template <int W, bool ToLds>
__device__ __forceinline__ void interleaved_side(uint8_t *I, int a, int L, uint32_t *lds) {
    uint8_t *base = I - a;  // (the 16-byte boundary in front of the span: dereferenced at offsets in [a, a + L) only)
    const int words = (a + L + 15) >> 4;
    for (int k = threadIdx.x; k < words; k += 256) {
        const int lo = 16 * k, hi = lo + 16;
        if (lo >= a && hi <= a + L) {
            if (ToLds) {
                const uint4 v = *(const uint4 *) (base + lo);
                lds[pad(lo) >> 2] = v.x, lds[(pad(lo) >> 2) + 1] = v.y, lds[(pad(lo) >> 2) + 2] = v.z, lds[(pad(lo) >> 2) + 3] = v.w;
            } else {
                const int d = pad(lo) >> 2;
                *(uint4 *) (base + lo) = make_uint4(lds[d], lds[d + 1], lds[d + 2], lds[d + 3]);
            }
            continue;
        }
        const int e0 = lo > a ? lo : a, e1 = hi < a + L ? hi : a + L;
        for (int o = e0; o < e1; o += W) {
            if (ToLds) lds_put<W>(lds, o, load_one<W>(base + o));
            else store_one<W>(base + o, lds_get<W>(lds, o));
        }
    }
}

// The channels' side: channel c's `cnt` elements of the span at P = planar row g C + c, sample t S.  Sample i of channel c sits at image
// offset a + (i C + c) W.  ToLds: the rows -> image, else back.
template <int W, bool ToLds>
__device__ __forceinline__ void channel_side(uint8_t *rows, long long grp, long long first, long long n, int C, int S, int cnt, int a, uint32_t *lds) {
    constexpr int E = 16 / W;
    const int wpc = S / E + 1, len = cnt * W;  // the aligned words that can cover a row's part of the span; its bytes
    for (int u = threadIdx.x; u < C * wpc; u += 256) {
        const int c = u / wpc, k = u - c * wpc;
        uint8_t *P = rows + ((size_t) (grp * C + c) * (size_t) n + (size_t) first) * W;
        const int p = (int) ((uintptr_t) P & 15);
        uint8_t *base = P - p;  // (dereferenced at offsets in [p, p + len) only)
        const int lo = 16 * k, hi = lo + 16;
        if (lo >= p && hi <= p + len) {
            const int at = a + (((lo - p) / W) * C + c) * W;
            if (ToLds) {
                const uint4 v = *(const uint4 *) (base + lo);
                const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < E; ++i) lds_put<W>(lds, at + i * C * W, get<W>(x, i));
            } else {
                uint32_t y[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < E; ++i) put<W>(y, i, lds_get<W>(lds, at + i * C * W));
                *(uint4 *) (base + lo) = make_uint4(y[0], y[1], y[2], y[3]);
            }
            continue;
        }
        const int e0 = lo > p ? lo : p, e1 = hi < p + len ? hi : p + len;
        for (int o = e0; o < e1; o += W) {
            const int at = a + (((o - p) / W) * C + c) * W;
            if (ToLds) lds_put<W>(lds, at, load_one<W>(base + o));
            else store_one<W>(base + o, lds_get<W>(lds, at));
        }
    }
}

template <int W, bool Join>
__device__ __forceinline__ void channel_span(const ChannelArgs &g) {
    __shared__ uint32_t lds[kChLds];
    const int C = g.C, S = ch_span(C, W);
    const long long spans = (g.n + S - 1) / S, grp = (long long) blockIdx.x / spans, first = ((long long) blockIdx.x % spans) * S;
    long long n = g.n;
    if (Join && g.counts) {
        n = g.counts[grp * C];
        n = n < 0 ? 0 : n > g.n ? g.n : n;
    }
    if (n <= first) return;  // (the whole workgroup: nothing of this span is delivered)
    const int cnt = n - first < S ? (int) (n - first) : S;
    uint8_t *I = (uint8_t *) (Join ? g.out : const_cast<void *>(g.in)) + ((size_t) grp * (size_t) g.n + (size_t) first) * C * W;
    uint8_t *rows = (uint8_t *) (Join ? const_cast<void *>(g.in) : g.out);
    const int a = (int) ((uintptr_t) I & 15), L = cnt * C * W;
    if (Join) channel_side<W, true>(rows, grp, first, g.n, C, S, cnt, a, lds);
    else interleaved_side<W, true>(I, a, L, lds);
    __syncthreads();
    if (Join) interleaved_side<W, false>(I, a, L, lds);
    else channel_side<W, false>(rows, grp, first, g.n, C, S, cnt, a, lds);
}

}  // namespace

template <int W>
__global__ __launch_bounds__(256) void channels_split_kernel(ChannelArgs g) {
    channel_span<W, false>(g);
}

template <int W>
__global__ __launch_bounds__(256) void channels_join_kernel(ChannelArgs g) {
    channel_span<W, true>(g);
}

template <int W>
static void launch_channels(bool join, const ChannelArgs &a, hipStream_t s) {
    const long long S = ch_span(a.C, W);
    const dim3 grid((unsigned) ((a.n + S - 1) / S * a.G));
    if (join) hipLaunchKernelGGL(channels_join_kernel<W>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(channels_split_kernel<W>, grid, dim3(256), 0, s, a);
}
static void launch_channels(int width, bool join, const ChannelArgs &a, hipStream_t s) {
    if (a.G <= 0 || a.n <= 0) return;
    if (width == 4) launch_channels<4>(join, a, s);
    else if (width == 2) launch_channels<2>(join, a, s);
    else launch_channels<1>(join, a, s);
}
void launch_channels_split(int width, const ChannelArgs &a, hipStream_t s) { launch_channels(width, false, a, s); }
void launch_channels_join(int width, const ChannelArgs &a, hipStream_t s) { launch_channels(width, true, a, s); }

}  // namespace kns
