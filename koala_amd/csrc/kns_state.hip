// kns_state.hip -- per-stream state between the engine's packed HBM layouts and the logical stream record (DESIGN.md section 4,
// "Stream record"; kns_kernels.h, StateArgs).  state_export_kernel gathers the listed streams' state out of the current ping-pong copies,
// state_import_kernel scatters records into BOTH copies (as reset_kernel does), so that no route, captured one-frame graph or in-place
// variant can read a stale one.  Plain HIP C++, vector loads and stores only.
//
// One workgroup serves FOUR consecutive rows (streams 16 mt + 4 q ... + 3) of one m-tile and keeps their four records in LDS (40 KiB
// for a one-frame front-end).  That is the grain at which every layout is contiguous: in a C-packed 16x16 tile the rows 4 q ... 4 q + 3
// are the float4 of lanes 16 q ... 16 q + 15 -- a 256-byte run of the 1 KiB tile -- so a wave's load covers those runs of four
// neighbouring tiles, every fetched byte is used, and the four workgroups of an m-tile read the whole tile between them.  The record
// side moves as contiguous 16-byte words (a wave: 1 KiB of one record).  A workgroup none of whose rows is listed returns after one
// 16-byte look at the table, so a sparse list costs its own m-tiles' traffic and nothing else.
#include "kns_kernels.h"

namespace kns {

namespace {

constexpr int kHdr4 = kStateHeaderBytes / 16, kHist4 = kFrame * 2 / 16, kTail4 = kFrame * 4 / 16;
constexpr int kHWord = kStateHOff / 4, kFctxWord = kStateFctxOff / 4;
constexpr int kStateTiles = kGruLayers * kUnitTiles;  // 136 hidden-state tiles per m-tile

// bit i: row 4 q + i of this workgroup is listed; rec[i]: its record
__device__ __forceinline__ unsigned listed_rows(const StateArgs &g, int b0, int (&rec)[4]) {
    const int4 r = *(const int4 *) (g.rec_of + b0);  // (b0 is a multiple of 4; the table has Bpad entries)
    rec[0] = r.x, rec[1] = r.y, rec[2] = r.z, rec[3] = r.w;
    return (r.x >= 0 ? 1u : 0u) | (r.y >= 0 ? 2u : 0u) | (r.z >= 0 ? 4u : 0u) | (r.w >= 0 ? 8u : 0u);
}

}  // namespace

__global__ __launch_bounds__(256) void state_export_kernel(StateArgs g) {
    extern __shared__ uint4 lds4[];  // [4 rows][state_bytes / 16]
    uint32_t *img = (uint32_t *) lds4;
    const int tid = threadIdx.x, mt = blockIdx.x >> 2, q = blockIdx.x & 3, mtiles = g.Bpad >> 4;
    const int b0 = mt * 16 + q * 4;
    int rec[4];
    const unsigned listed = listed_rows(g, b0, rec);
    if (!listed) return;
    const int W4 = (int) (g.state_bytes >> 4), W = W4 * 4;

    if (tid < 4 * kHdr4) lds4[(tid >> 1) * W4 + (tid & 1)] = (tid & 1) ? g.hdr1 : g.hdr0;
    if (tid < 4 * kHist4) {
        const int i = tid / kHist4, w = tid % kHist4;
        lds4[i * W4 + kStateHistOff / 16 + w] = ((const uint4 *) (g.hist[0] + (size_t) (b0 + i) * kFrame))[w];
    }
    {
        const int i = tid / kTail4, w = tid % kTail4;  // 4 x 64 words: one per thread
        lds4[i * W4 + kStateTailOff / 16 + w] = ((const uint4 *) (g.tail[0] + (size_t) (b0 + i) * kFrame))[w];
    }
    {   // (front_taps 2 ... 4: the record is padded up to whole 16-byte words, with zeros)
        const int pad = W - (kFctxWord + (g.taps - 1) * kBins);
        if (tid < 4 * pad) img[(tid / pad) * W + W - pad + tid % pad] = 0;
    }
    // hidden state: lane group c of tile (layer, u) holds column c of the four rows
    for (int idx = tid; idx < kStateTiles * 16; idx += 256) {
        const int tile = idx >> 4, c = idx & 15, layer = tile / kUnitTiles, u = tile - layer * kUnitTiles;
        const float4 v = *(const float4 *) (g.hstate[0] + (((size_t) layer * mtiles + mt) * kUnitTiles + u) * 256 + (q * 16 + c) * 4);
        const int k = u * 16 + c;
        if (k < kHidden) {
            uint32_t *p = img + kHWord + layer * kHidden + k;
            p[0] = __float_as_uint(v.x), p[W] = __float_as_uint(v.y), p[2 * W] = __float_as_uint(v.z), p[3 * W] = __float_as_uint(v.w);
        }
    }
    // feature context: record frame f is slot f + 1 of the history; a row of an A-packed block is the 16-byte words of lanes
    // row, row + 16, row + 32, row + 48
    for (int it = tid; it < (g.taps - 1) * g.nbf * 16; it += 256) {
        const int f = it / (g.nbf * 16), rem = it - f * g.nbf * 16, kb = rem >> 4, i = (rem >> 2) & 3, gq = rem & 3;
        const uint4 wv = ((const uint4 *) g.fhist)[(((size_t) (f + 1) * mtiles + mt) * g.nbf + kb) * 64 + q * 4 + i + 16 * gq];
        uint32_t *p = img + i * W + kFctxWord + f * kBins;
        const uint32_t e[4] = {wv.x, wv.y, wv.z, wv.w};
        if (g.precision == kBf16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kb * 32 + gq * 8 + j;
                if (k < kBins) p[k] = (j & 1) ? (e[j >> 1] & 0xffff0000u) : (e[j >> 1] << 16);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kb * 16 + j * 4 + gq;
                if (k < kBins) p[k] = e[j];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (rec[i] < 0) continue;
        uint4 *dst = (uint4 *) (g.records + (size_t) rec[i] * g.state_bytes);
        for (int w = tid; w < W4; w += 256) dst[w] = lds4[i * W4 + w];
    }
}

__global__ __launch_bounds__(256) void state_import_kernel(StateArgs g) {
    extern __shared__ uint4 lds4[];
    const uint32_t *img = (const uint32_t *) lds4;
    const int tid = threadIdx.x, mt = blockIdx.x >> 2, q = blockIdx.x & 3, mtiles = g.Bpad >> 4;
    const int b0 = mt * 16 + q * 4;
    int rec[4];
    const unsigned listed = listed_rows(g, b0, rec);
    if (!listed) return;
    const int W4 = (int) (g.state_bytes >> 4), W = W4 * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (rec[i] < 0) continue;
        const uint4 *src = (const uint4 *) (g.records + (size_t) rec[i] * g.state_bytes);
        for (int w = tid; w < W4; w += 256) lds4[i * W4 + w] = src[w];
    }
    __syncthreads();

    if (tid < 4 * kHist4) {
        const int i = tid / kHist4, w = tid % kHist4;
        if (listed >> i & 1) {
            const uint4 v = lds4[i * W4 + kStateHistOff / 16 + w];
            ((uint4 *) (g.hist[0] + (size_t) (b0 + i) * kFrame))[w] = v;
            ((uint4 *) (g.hist[1] + (size_t) (b0 + i) * kFrame))[w] = v;
        }
    }
    {
        const int i = tid / kTail4, w = tid % kTail4;
        if (listed >> i & 1) {
            const uint4 v = lds4[i * W4 + kStateTailOff / 16 + w];
            ((uint4 *) (g.tail[0] + (size_t) (b0 + i) * kFrame))[w] = v;
            ((uint4 *) (g.tail[1] + (size_t) (b0 + i) * kFrame))[w] = v;
        }
    }
    // hidden state: the float4 of a lane is one column of the four rows -- a whole store where all four are listed, else the listed
    // rows' components; column 271 (padding of unit tile 16) is left as the engine keeps it
    for (int idx = tid; idx < kStateTiles * 16; idx += 256) {
        const int tile = idx >> 4, c = idx & 15, layer = tile / kUnitTiles, u = tile - layer * kUnitTiles;
        const int k = u * 16 + c;
        if (k >= kHidden) continue;
        const uint32_t *p = img + kHWord + layer * kHidden + k;
        const float4 v = make_float4(__uint_as_float(p[0]), __uint_as_float(p[W]), __uint_as_float(p[2 * W]), __uint_as_float(p[3 * W]));
        const size_t off = (((size_t) layer * mtiles + mt) * kUnitTiles + u) * 256 + (q * 16 + c) * 4;
        float *d0 = g.hstate[0] + off, *d1 = g.hstate[1] + off;
        if (listed == 15u) {
            *(float4 *) d0 = v;
            *(float4 *) d1 = v;
        } else {
            if (listed & 1u) d0[0] = v.x, d1[0] = v.x;
            if (listed & 2u) d0[1] = v.y, d1[1] = v.y;
            if (listed & 4u) d0[2] = v.z, d1[2] = v.z;
            if (listed & 8u) d0[3] = v.w, d1[3] = v.w;
        }
    }
    // feature context: a 16-byte word of the history belongs to one row; a word that reaches into the padding columns (257 ...) has
    // only its valid elements stored
    for (int it = tid; it < (g.taps - 1) * g.nbf * 16; it += 256) {
        const int f = it / (g.nbf * 16), rem = it - f * g.nbf * 16, kb = rem >> 4, i = (rem >> 2) & 3, gq = rem & 3;
        if (!(listed >> i & 1)) continue;
        const uint32_t *p = img + i * W + kFctxWord + f * kBins;
        uint4 *dst = (uint4 *) g.fhist + (((size_t) (f + 1) * mtiles + mt) * g.nbf + kb) * 64 + q * 4 + i + 16 * gq;
        if (g.precision == kBf16) {
            const int k0 = kb * 32 + gq * 8;
            if (k0 + 8 <= kBins) {
                uint4 v;
                v.x = (p[k0] >> 16) | (p[k0 + 1] & 0xffff0000u);
                v.y = (p[k0 + 2] >> 16) | (p[k0 + 3] & 0xffff0000u);
                v.z = (p[k0 + 4] >> 16) | (p[k0 + 5] & 0xffff0000u);
                v.w = (p[k0 + 6] >> 16) | (p[k0 + 7] & 0xffff0000u);
                *dst = v;
            } else {
                for (int j = 0; j < 8 && k0 + j < kBins; ++j) ((uint16_t *) dst)[j] = (uint16_t) (p[k0 + j] >> 16);
            }
        } else {
            const int k0 = kb * 16 + gq;
            if (k0 + 12 < kBins) {
                *dst = make_uint4(p[k0], p[k0 + 4], p[k0 + 8], p[k0 + 12]);
            } else {
                for (int j = 0; j < 4 && k0 + 4 * j < kBins; ++j) ((uint32_t *) dst)[j] = p[k0 + 4 * j];
            }
        }
    }
}

void launch_state_export(const StateArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(state_export_kernel, dim3(a.Bpad / 4), dim3(256), 4 * (size_t) a.state_bytes, s, a);
}

void launch_state_import(const StateArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(state_import_kernel, dim3(a.Bpad / 4), dim3(256), 4 * (size_t) a.state_bytes, s, a);
}

}  // namespace kns
