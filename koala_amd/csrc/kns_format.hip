// kns_format.hip -- the sample formats of batch handles (fifth extension; section 6): float32 and G.711 samples
// converted on the device around the unchanged int16 call.  Plain HIP C++, vector loads and stores only, no table: the codecs are shifts, a
// count of leading zeros for the segment and the float conversions.
//
// format_in_kernel<Fmt>:  the caller's elements -> the engine's int16 samples (every element of every row)
// format_out_kernel<Fmt>: the engine's int16 samples -> the caller's elements; a packet call writes row b's first counts[b] elements only
//
// Both are one routine over rows of n elements: one lane converts one group of G = 16 (8-bit formats) or 8 (float) elements whose
// DESTINATION is 16-byte aligned -- one or two aligned 16-byte stores.  The group's source bytes sit at some byte offset a of an aligned
// 16-byte word (a caller's pointer is aligned to its element only; rows of an odd length shift by row): the lane loads the aligned words
// that cover them and funnel-shifts by a, which is uniform over a row.  A row's ragged head (up to its destination's first aligned
// address) and tail (less than a group), and a group whose covering source words would reach outside the source matrix, go per sample.
#include "kns_kernels.h"

namespace kns {

namespace {

__device__ __forceinline__ float u2f(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
__device__ __forceinline__ uint32_t f2u(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// dec: an element's bits -> the int16 sample; enc: an int16 sample -> the element's bits (the table of the formats)
template <int Fmt>
struct Codec;
template <>
struct Codec<kFmtF32> {
    static __device__ __forceinline__ int dec(uint32_t bits) {
        const float x = u2f(bits);
        if (x != x) return 0;
        // (the product is exact or +-inf; step 4's rounding: half away from zero, then the clip)
        return (int) __builtin_fminf(__builtin_fmaxf(__builtin_roundf(x * 32768.0f), -32768.0f), 32767.0f);
    }
    static __device__ __forceinline__ uint32_t enc(int s) { return f2u((float) s * (1.0f / 32768)); }
};
template <>
struct Codec<kFmtUlaw> {
    static __device__ __forceinline__ int dec(uint32_t b) {
        const uint32_t u = ~b & 0xFF;
        const int e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84;
        return (u & 0x80) ? -mag : mag;
    }
    static __device__ __forceinline__ uint32_t enc(int s) {
        const uint32_t sign = s < 0 ? 0x80 : 0;
        const int abs_s = s < 0 ? -s : s, mag = (abs_s < 32635 ? abs_s : 32635) + 0x84;  // 0x84 ... 0x7FFF: 8 to 15 bits
        const int e = 24 - __builtin_clz((unsigned) mag), m = (mag >> (e + 3)) & 15;
        return ~(sign | (uint32_t) (e << 4) | (uint32_t) m) & 0xFF;
    }
};
template <>
struct Codec<kFmtAlaw> {
    static __device__ __forceinline__ int dec(uint32_t b) {
        const uint32_t a = (b ^ 0x55) & 0xFF;
        const int e = (a >> 4) & 7, m = a & 15, mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
        return (a & 0x80) ? mag : -mag;
    }
    static __device__ __forceinline__ uint32_t enc(int s) {
        const uint32_t sign = s >= 0 ? 0x80 : 0;
        const int mag = s >= 0 ? s : ~s;
        const int e = mag < 256 ? 0 : 24 - __builtin_clz((unsigned) mag), m = e == 0 ? (mag >> 4) & 15 : (mag >> (e + 3)) & 15;
        return (sign | (uint32_t) (e << 4) | (uint32_t) m) ^ 0x55;
    }
};

// element i of a packed group of W-byte elements (the low 8 W bits of the result / of `bits`)
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
template <int W>
__device__ __forceinline__ uint32_t load_one(const uint8_t *p, long long i) {
    if (W == 4) return ((const uint32_t *) p)[i];
    if (W == 2) return ((const uint16_t *) p)[i];
    return p[i];
}
template <int W>
__device__ __forceinline__ void store_one(uint8_t *p, long long i, uint32_t bits) {
    if (W == 4) ((uint32_t *) p)[i] = bits;
    else if (W == 2) ((uint16_t *) p)[i] = (uint16_t) bits;
    else p[i] = (uint8_t) bits;
}
// one source element's bits -> the destination element's bits
template <int Fmt, bool In>
__device__ __forceinline__ uint32_t convert(uint32_t bits) {
    if (In) return (uint32_t) Codec<Fmt>::dec(bits) & 0xFFFF;
    return Codec<Fmt>::enc((int) (int16_t) bits);
}
template <int Fmt, bool In>
__device__ __forceinline__ void format_rows(const FormatArgs &g) {
    constexpr int EB = Fmt == kFmtF32 ? 4 : 1, SB = In ? EB : 2, DB = In ? 2 : EB;  // bytes per source / destination element
    constexpr int G = Fmt == kFmtF32 ? 8 : 16, SW = G * SB / 16, DW = G * DB / 16;   // a group, and its 16-byte words on either side
    const long long bpr = (g.n / G + 2 + 255) / 256;  // workgroups per row: one lane for the head, one per group, one for the tail
    const long long row = (long long) blockIdx.x / bpr, lane = ((long long) blockIdx.x % bpr) * 256 + threadIdx.x;
    long long cnt = g.n;
    if (g.counts) {
        cnt = g.counts[row];
        cnt = cnt < 0 ? 0 : cnt > g.n ? g.n : cnt;
    }
    const uint8_t *S = (const uint8_t *) g.in + (size_t) row * g.n * SB;
    uint8_t *D = (uint8_t *) g.out + (size_t) row * g.n * DB;
    long long h = (long long) (((16 - ((uintptr_t) D & 15)) & 15) / DB);  // the elements in front of D's first aligned address
    if (h > cnt) h = cnt;
    const long long ng = (cnt - h) / G;
    long long e0 = 0, e1 = h;
    if (lane > 0) {
        const long long j = lane - 1;
        if (j > ng) return;
        e0 = h + j * G;
        e1 = j < ng ? e0 + G : cnt;
    }
    if (lane > 0 && e1 - e0 == G) {
        const uintptr_t a = (uintptr_t) (S + e0 * SB) & 15;
        const uint8_t *wp = S + e0 * SB - a;                                            // the aligned word the group's first byte is in
        const uint8_t *lo = (const uint8_t *) g.in, *hi = lo + (size_t) g.rows * g.n * SB;  // the source matrix
        if ((uintptr_t) wp >= (uintptr_t) lo && (uintptr_t) wp + 16 * (SW + (a ? 1 : 0)) <= (uintptr_t) hi) {
            uint32_t w[4 * SW + 4], t[4 * SW + 3], u[4 * SW + 1], x[4 * SW], y[4 * DW];
#pragma unroll
            for (int k = 0; k < SW; ++k) {
                const uint4 v = *(const uint4 *) (wp + 16 * k);
                w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
            }
            uint4 last = make_uint4(0, 0, 0, 0);
            if (a) last = *(const uint4 *) (wp + 16 * SW);
            w[4 * SW] = last.x, w[4 * SW + 1] = last.y, w[4 * SW + 2] = last.z, w[4 * SW + 3] = last.w;
            // x = the group's bytes: w moved down by a bytes -- by one word, by two words, then by bits.  (The two selects are written as
            // masks: given a ?: over neighbouring elements the compiler indexes the array, which puts it into scratch.)
            const int r8 = (int) (a & 3) * 8;
            const uint32_t m1 = (a & 4) ? ~0u : 0u, m2 = (a & 8) ? ~0u : 0u;
#pragma unroll
            for (int k = 0; k < 4 * SW + 3; ++k) t[k] = w[k] ^ ((w[k] ^ w[k + 1]) & m1);
#pragma unroll
            for (int k = 0; k < 4 * SW + 1; ++k) u[k] = t[k] ^ ((t[k] ^ t[k + 2]) & m2);
#pragma unroll
            for (int k = 0; k < 4 * SW; ++k) x[k] = (uint32_t) ((((uint64_t) u[k + 1] << 32) | u[k]) >> r8);
#pragma unroll
            for (int k = 0; k < 4 * DW; ++k) y[k] = 0;
#pragma unroll
            for (int i = 0; i < G; ++i) put<DB>(y, i, convert<Fmt, In>(get<SB>(x, i)));
#pragma unroll
            for (int k = 0; k < DW; ++k) *(uint4 *) (D + e0 * DB + 16 * k) = make_uint4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
            return;
        }
    }
    for (long long e = e0; e < e1; ++e) store_one<DB>(D, e, convert<Fmt, In>(load_one<SB>(S, e)));
}

}  // namespace

template <int Fmt>
__global__ __launch_bounds__(256) void format_in_kernel(FormatArgs g) {
    format_rows<Fmt, true>(g);
}

template <int Fmt>
__global__ __launch_bounds__(256) void format_out_kernel(FormatArgs g) {
    format_rows<Fmt, false>(g);
}

template <int Fmt>
static void launch_format(bool in, const FormatArgs &a, hipStream_t s) {
    const long long bpr = (a.n / fmt_group(Fmt) + 2 + 255) / 256;
    const dim3 grid((unsigned) (bpr * a.rows));
    if (in) hipLaunchKernelGGL(format_in_kernel<Fmt>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(format_out_kernel<Fmt>, grid, dim3(256), 0, s, a);
}
static void launch_format(int fmt, bool in, const FormatArgs &a, hipStream_t s) {
    if (a.rows <= 0 || a.n <= 0) return;
    if (fmt == kFmtF32) launch_format<kFmtF32>(in, a, s);
    else if (fmt == kFmtUlaw) launch_format<kFmtUlaw>(in, a, s);
    else launch_format<kFmtAlaw>(in, a, s);
}
void launch_format_in(int fmt, const FormatArgs &a, hipStream_t s) { launch_format(fmt, true, a, s); }
void launch_format_out(int fmt, const FormatArgs &a, hipStream_t s) { launch_format(fmt, false, a, s); }

}  // namespace kns
