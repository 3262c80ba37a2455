// kns_stft.hip -- analysis (int16 -> STFT -> features), synthesis (mask x spectrum -> iSTFT -> OLA -> int16) and state reset;
// SURVEY.md 8a rows a2, a3, a5, a6.  See kns_kernels.h for the launch interface.
#include "kns_device.hpp"

namespace kns {

// ------------------------------------------------------------------------------------------------ shared pieces

// One row of 16 lanes owns one stream; a wave four streams; a workgroup (4 waves) the 16 streams of an m-tile.
// The lane in column c of its row (c = fft_column(lane), kns_device.hpp) holds the 16 points n = c + 16 j of whatever
// 256-point complex sequence is live: packed samples z[n] = x[2n] + i x[2n+1], FFT bins, inverse-FFT input.  Every table
// the lane needs is indexed by such n, so it sits in LDS in natural order and is read at (lane base + immediate offset).
constexpr int kOffTw = 0;                               // float2[512]: exp(-2 pi i k / 512)
constexpr int kOffWin = 4096;                           // float[512]:  sin(pi n / 512) / 32768 (analysis: int16 -> windowed sample)
constexpr int kOffWinS = kOffWin + 2048;                // float[512]:  sin(pi n / 512) / 256   (synthesis: FFT sum -> windowed sample)
constexpr int kOffTwl = kOffWinS + 2048;                // fft_fill_twiddles table
constexpr int kOffXbuf = kOffTwl + kFftTwiddleBytes;    // 4 waves x kFftWaveBytes
constexpr int kOffStftEnd = kOffXbuf + 4 * kFftWaveBytes;

// kSynth: also the synthesis window.  (The analysis kernel leaves that table out and puts its exchange tiles there: 2 KiB
// decide whether three of its workgroups fit a CU's 160 KiB.)
// The tables of a workgroup, requested by its 256 STFT threads in ONE go and stored to LDS when they are there (as loops of
// load -> store, hipcc waited for every load before the next one was requested: five memory round trips at the head of every
// launch, most of a one-frame call's STFT kernels).
struct StftTables {
    float2 tw[2];
    float win[2];
    float2 twl;
};
__device__ __forceinline__ void stft_request_tables(StftTables &t, const float *twiddle, const float *window, int tid) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        t.tw[q] = ((const float2 *) twiddle)[tid + 256 * q];
        t.win[q] = window[tid + 256 * q];
    }
    t.twl = ((const float2 *) twiddle)[2 * (((tid & 15) * (tid >> 4)) & 255)];  // fft_fill_twiddles' entry of this thread
}
template <bool kSynth>
__device__ __forceinline__ void stft_store_tables(const StftTables &t, char *smem, int tid) {
    float2 *tw = (float2 *) (smem + kOffTw);
    float *win = (float *) (smem + kOffWin), *wins = (float *) (smem + kOffWinS);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + 256 * q;
        tw[i] = t.tw[q];
        // the powers of two of the spec's (x / 32768) w and (y / 256) w are folded into the window: exact, so the
        // products are the spec's bit for bit
        win[i] = t.win[q] * (1.0f / 32768.0f);
        if (kSynth) wins[i] = t.win[q] * (1.0f / 256.0f);
    }
    ((float2 *) (smem + (kSynth ? kOffTwl : kOffWinS)))[tid] = t.twl;
}
// analysis kernel: [tw | win | fft twiddles | exchange tiles | mean, scale | feature tile]
constexpr int kOffATwl = kOffWinS, kOffAXbuf = kOffATwl + kFftTwiddleBytes, kOffAEnd = kOffAXbuf + 4 * kFftWaveBytes;

// the eight dwords (sample pairs) this lane owns of one 256-sample frame: pairs 16 jj + c
__device__ __forceinline__ void load_frame(int (&f)[8], const int16_t *frame, int c) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) f[jj] = ((const int *) frame)[16 * jj + c];
}

// windowed packed samples of the 512-sample analysis block [prev | cur]; win_c = LDS window + 8 c
__device__ __forceinline__ void window_block(cpx (&v)[16], const int (&prev)[8], const int (&cur)[8], const char *win_c) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int pr = j < 8 ? prev[j] : cur[j - 8];
        const float2 w = *(const float2 *) (win_c + j * 128);  // window[2n], window[2n + 1], n = 16 j + c
        const float lo = (float) (int16_t) (pr & 0xffff), hi = (float) (int16_t) (pr >> 16);
        v[j].x = lo * w.x;  // = (lo / 32768) window[2n]: the window table carries the 2^-15
        v[j].y = hi * w.y;
    }
}

// Half spectrum of the real 512-point block from the 256-point FFT Z of its packed samples: X[k], k = c + 16 k2.
// Bin 0 carries {X[0], X[256]} (both real).  The arithmetic is the same in the analysis and the synthesis kernel, so a
// spectrum that is recomputed instead of stored is the stored one bit for bit.  tw_c = LDS exp(-2 pi i k / 512) + 8 c.
__device__ __forceinline__ void real_spectrum(const cpx (&z)[16], cpx (&x)[16], const char *tw_c, int c) {
    cpx zp[16];
    fft_partner(z, zp, c);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
        const cpx zk = z[k2];
        const float2 w = *(const float2 *) (tw_c + k2 * 128);
        // s = Z[k] + conj(Z[256 - k]), d = Z[k] - conj(Z[256 - k])
        const cpx s = {zk.x + zp[k2].x, zk.y - zp[k2].y}, d = {zk.x - zp[k2].x, zk.y + zp[k2].y};
        const cpx p = cmul(d, cpx{w.x, w.y});
        cpx r = {0.5f * (s.x + p.y), 0.5f * (s.y - p.x)};
        if (k2 == 0 && c == 0) r = cpx{zk.x + zk.y, zk.x - zk.y};
        x[k2] = r;
    }
}

// ------------------------------------------------------------------------------------------------ analysis

template <class P>
__device__ __forceinline__ float feature_log(float x) {
    // fp32 configuration: the spec's full-precision polynomial.  bf16 configuration: the feature is rounded to bf16 (8 bits) right
    // after, so a short polynomial serves -- an exactly reproducible one (kns_log_fast), not the hardware logarithm: the features of
    // the two configurations are each bit-identical to the oracle's.
    if (P::kPrec == kBf16) return kns_log_fast(x);
    return kns_log(x);
}

// grid (stream tiles, time segments): a workgroup walks the frames [t0, t1) of its 16 streams, so every PCM sample is
// read once (the previous frame stays in registers) and the per-lane constants are set up once per segment.
// kResets: calls with per-frame stream resets (AnalysisArgs::resets): in a row's reset frame the previous frame is zero -- the block
// [0 | frame t] a fresh stream sees -- and a segment whose first frame is one does not read the frame in front of it
template <class P, bool kSpec, bool kResets = false>
__global__ __launch_bounds__(256, 3) void analysis_kernel(AnalysisArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *lmean = (float *) (smem + kOffAEnd), *lscale = lmean + 272;
    typename P::elem_t *tile = (typename P::elem_t *) (smem + kOffAEnd + 2 * 272 * 4);  // nbf KiB

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = fft_column(lane), q = lane >> 4, row = wave * 4 + q;
    const int mt = blockIdx.x, mtiles = g.Bpad >> 4;
    const int t0 = blockIdx.y * g.seg, t1 = min(g.T, t0 + g.seg);
    const int b = mt * 16 + row;
    const size_t row_len = (size_t) (g.pitch ? g.pitch : g.T) * kFrame;
    // rows past the last stream (ragged last tile) read the last stream's samples: their results are never stored
    // anywhere a stream would see them, and the loop carries no conditional vector-memory operation
    const int16_t *pcm_row = g.pcm + (size_t) (b < g.B ? b : g.B - 1) * row_len;

    // (one-frame calls of a several-frame front-end) this m-tile's feature history, slots 1 .. hist_slots, on its way to LDS; it
    // goes back one slot down after the first barrier, when all of it has been read
    char *hroll = smem + kOffAEnd + 2 * 272 * 4 + (size_t) g.nbf * 1024;
    if (g.feat_hist) {
        typedef const __attribute__((address_space(1))) void *gptr_t;
        typedef __attribute__((address_space(3))) void *lptr_t;
        for (int i = wave; i < g.hist_slots * g.nbf; i += 4) {
            const int slot = i / g.nbf, kb = i - slot * g.nbf;
            __builtin_amdgcn_global_load_lds(
                (gptr_t) ((const uint4 *) g.feat_hist + (((size_t) (slot + 1) * mtiles + mt) * g.nbf + kb) * 64 + lane),
                (lptr_t) (hroll + i * 1024), 16, 0, 0);
        }
    }
    int prev[8], cur[8], nxt[8];
    // (a slice of a longer call, prev_in_pcm: the frame in front of frame 0 sits in the row itself, at t = -1)
    if (kResets && ((reset_rows(g.resets, g.rs_pitch, mt, g.rs_t0 + t0) >> row) & 1u)) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) prev[jj] = 0;
    } else {
        load_frame(prev, t0 == 0 && !g.prev_in_pcm ? g.hist_in + (size_t) b * kFrame : pcm_row + ((ptrdiff_t) t0 - 1) * kFrame, c);
    }
    load_frame(cur, pcm_row + (size_t) t0 * kFrame, c);
    StftTables tbl;
    stft_request_tables(tbl, g.twiddle, g.window, tid);
    float ms[2][2];  // mean, scale of bins tid and tid + 256 (clamped: 257 bins)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + 256 * q < kBins ? tid + 256 * q : kBins - 1;
        ms[q][0] = g.mean[i];
        ms[q][1] = g.scale[i];
    }
    stft_store_tables<false>(tbl, smem, tid);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + 256 * q;
        if (i < kBins) {
            lmean[i] = ms[q][0];
            lscale[i] = ms[q][1];
        }
    }
    {
        uint4 *z = (uint4 *) tile;
        for (int i = tid; i < g.nbf * 64; i += 256) z[i] = uint4{0, 0, 0, 0};
    }
    __syncthreads();
    if (g.feat_hist) {
        for (int i = tid; i < g.hist_slots * g.nbf * 64; i += 256) {
            const int slot = i / (g.nbf * 64), w = i - slot * g.nbf * 64;
            ((uint4 *) g.feat_hist)[((size_t) slot * mtiles + mt) * g.nbf * 64 + w] = ((const uint4 *) hroll)[i];
        }
    }
    char *xw;
    const char *xr, *twl_c;
    fft_lane_bases(smem + kOffAXbuf + wave * kFftWaveBytes, smem + kOffATwl, lane, &xw, &xr, &twl_c);
    const char *tw_c = smem + kOffTw + c * 8, *win_c = smem + kOffWin + c * 8;
    const float *mean_c = lmean + c, *scale_c = lscale + c;

    for (int t = t0; t < t1; ++t) {
        // next frame's samples are requested before this frame is transformed (clamped, never skipped)
        load_frame(nxt, pcm_row + (size_t) (t + 1 < t1 ? t + 1 : t) * kFrame, c);
        if (kResets && t > t0) {  // (the segment's first frame was taken care of above)
            const unsigned rm = reset_rows(g.resets, g.rs_pitch, mt, g.rs_t0 + t);
            if (rm) {
                const bool r = (rm >> row) & 1u;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) prev[jj] = r ? 0 : prev[jj];
            }
        }
        cpx v[16];
        window_block(v, prev, cur, win_c);
        fft256_rows(v, twl_c, xw, xr);
        cpx x[16];
        real_spectrum(v, x, tw_c, c);
        if (kSpec) {
            // stored in the lane order of this kernel pair: bins (c + 16 k2, c + 16 (k2 + 1)), k2 even, as one 16-byte word
            // at [(k2 / 2) * 16 + c] -- a row of lanes moves 256 contiguous bytes per instruction
            f32x4 *spec = (f32x4 *) g.spec + ((size_t) t * g.Bpad + b) * 128;
#pragma unroll
            for (int k2 = 0; k2 < 16; k2 += 2) spec[(k2 >> 1) * 16 + c] = f32x4{x[k2].x, x[k2].y, x[k2 + 1].x, x[k2 + 1].y};
        }
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            const int k = c + 16 * k2;
            float pw = __builtin_fmaf(x[k2].x, x[k2].x, x[k2].y * x[k2].y);
            if (k2 == 0 && c == 0) pw = x[k2].x * x[k2].x;
            const float ft = (feature_log<P>(pw + 1e-10f) - mean_c[16 * k2]) * scale_c[16 * k2];
            tile[(k / P::KB) * 64 * P::EPL + P::off(row, k % P::KB)] = P::cvt(ft);
        }
        if (c == 0) {  // Nyquist bin: the imaginary slot of bin 0
            const float nyq = x[0].y;
            const float fn = (feature_log<P>(nyq * nyq + 1e-10f) - lmean[256]) * lscale[256];
            tile[(256 / P::KB) * 64 * P::EPL + P::off(row, 256 % P::KB)] = P::cvt(fn);
        }
        __syncthreads();
        {
            const uint4 *src = (const uint4 *) tile;
            uint4 *dst = (uint4 *) g.feat + ((size_t) t * mtiles + mt) * g.nbf * 64;
            for (int i = tid; i < g.nbf * 64; i += 256) dst[i] = src[i];
        }
        __syncthreads();  // (a single tile and two barriers per frame: a second tile would cost the third workgroup per CU)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            prev[jj] = cur[jj];
            cur[jj] = nxt[jj];
        }
    }
    if (t1 == g.T && b < g.B && g.write_hist) {  // history for the next call: the last frame (prev after the final rotation)
        int *h = (int *) (g.hist_out + (size_t) b * kFrame);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) h[16 * jj + c] = prev[jj];
    }
}

void launch_analysis(const AnalysisArgs &a, hipStream_t s) {
    dim3 grid(a.Bpad / 16, (a.T + a.seg - 1) / a.seg);
    const size_t roll = a.feat_hist ? (size_t) a.hist_slots * a.nbf * 1024 : 0;  // (one-frame calls: one workgroup per CU is plenty)
#ifndef KNS_STFT_LDS_PAD  // timing experiment: extra dynamic LDS per workgroup = fewer workgroups per CU
#define KNS_STFT_LDS_PAD 0
#endif
    const size_t lds = kOffAEnd + 2 * 272 * 4 + (size_t) a.nbf * 1024 + roll + KNS_STFT_LDS_PAD;
    auto go = [&](auto kernel, int threads, size_t bytes) {
        if (bytes > 48 * 1024) (void) hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
        hipLaunchKernelGGL(kernel, grid, dim3(threads), bytes, s, a);
    };
    if (a.resets) {  // (calls with per-frame stream resets: the reset arm)
        if (a.precision == kBf16)
            a.write_spec ? go(analysis_kernel<PBF16, true, true>, 256, lds) : go(analysis_kernel<PBF16, false, true>, 256, lds);
        else
            a.write_spec ? go(analysis_kernel<PF32, true, true>, 256, lds) : go(analysis_kernel<PF32, false, true>, 256, lds);
    } else if (a.precision == kBf16) {
        if (a.write_spec)
            go(analysis_kernel<PBF16, true>, 256, lds);
        else
            go(analysis_kernel<PBF16, false>, 256, lds);
    } else {
        if (a.write_spec)
            go(analysis_kernel<PF32, true>, 256, lds);
        else
            go(analysis_kernel<PF32, false>, 256, lds);
    }
}

// ------------------------------------------------------------------------------------------------ synthesis

// grid (stream tiles, time segments); a workgroup produces frames [t0, t1) of its 16 streams.  A segment that does not
// start at 0 first replays frame t0 - 1 (no output) to rebuild the overlap-add tail it inherits.
// kRecompute: the spectrum of a frame is rebuilt from its 512 B of PCM (one more FFT in registers) instead of being read
// back as 2 KiB of fp32 that the analysis kernel would have had to write: the arithmetic is the analysis kernel's, so
// the result is the same bit for bit.  The stored form remains for single-frame calls, where the analysis kernel
// updates the history in place and the previous frame is gone by the time this kernel runs.
// (three waves per SIMD: the kernel is bound by VALU issue, and two waves on a SIMD reach an instruction every ~2.8 cycles,
// three come close to the pipe's 2; the register budget of 168 is what decides which loads are prefetched below)
// kMaskIn (one-frame calls, bf16): waves 4..7 are the mask head -- sigmoid(h . W_mask + b_mask) of the workgroup's m-tile as fp16 C
// fragments in LDS (what gemm_kernel<kOutMask> stores), complete at the workgroup's one barrier; the STFT waves read it from there.
// kResets (calls with per-frame stream resets, SynthesisArgs::resets): in a row's reset frame its overlap-add tail is zero and, recomputed,
// its spectrum is that of [0 | frame t].  This holds for the replayed frame t0 - 1 as well, and a reset at t0 zeroes the tail the replay
// left: nothing of the frames before a reset reaches the output.
// kMinGain (handles with a per-stream attenuation limit in force, SynthesisArgs::min_gain): the mask value m of every bin becomes
// m' = g + (1 - g) m, g the row's minimum gain -- one (g, 1 - g) pair per lane, loaded in front of the frame loop; DESIGN.md section 2, step 4.
// m' = g + u m of the spec: the product rounded, then the sum -- never one fused operation, whatever the build's flags say
__device__ __forceinline__ float min_gain_mask(float g, float u, float m) {
#pragma clang fp contract(off)
    const float p = u * m;
    return g + p;
}

// kLink (SynthesisArgs::link; the linked kernels below): the max of two mask values.  They are sigmoids: finite and not below +0, where the order of the bit patterns is the order of the values -- one
// v_max_i32, exact; fmaxf on values that come straight from memory is three v_max_f32 in IEEE mode (it quiets each operand first)
__device__ __forceinline__ float link_max(float a, float b) {
    const int x = __builtin_bit_cast(int, a), y = __builtin_bit_cast(int, b);
    return __builtin_bit_cast(float, __builtin_elementwise_max(x, y));
}

// kProfile (SynthesisArgs::profile; the profile kernels below): m' held between a bin's floor and ceiling, the max first.  All three are finite
// and not below +0 (m' = g + (1 - g) m of a sigmoid; the owner stores +0 for -0), where the order of the bit patterns is the order of the
// values: one v_max_i32 and one v_min_i32, exact, as link_max
__device__ __forceinline__ float profile_clamp(float lo, float hi, float m) {
    const int x = __builtin_elementwise_max(__builtin_bit_cast(int, m), __builtin_bit_cast(int, lo));
    return __builtin_bit_cast(float, __builtin_elementwise_min(x, __builtin_bit_cast(int, hi)));
}

// kComfort (SynthesisArgs::comfort_amp; the comfort kernels below; DESIGN.md section 2, twelfth extension): the variates of bin k of the
// frame with counter value n -- base = seed ^ (n * 0x9E3779B9) -- are the two halves of one hashed word, uniform in (-1, 1), exact in fp32;
// w = 1 - m', a = w A, Y = (m' X) + (a z): every operation rounded on its own, never fused, whatever the build's flags say
__device__ __forceinline__ unsigned comfort_hash(unsigned base, unsigned k) {
    unsigned v = base ^ (k * 0x85EBCA6Bu);
    v ^= v >> 16;
    v *= 0x7FEB352Du;
    v ^= v >> 15;
    v *= 0x846CA68Bu;
    v ^= v >> 16;
    return v;
}
__device__ __forceinline__ float comfort_variate(unsigned half) { return ((float) half - 32767.5f) * (1.0f / 32768.0f); }
__device__ __forceinline__ float comfort_amplitude(float m, float amp) {
#pragma clang fp contract(off)
    const float w = 1.0f - m;
    return w * amp;
}
__device__ __forceinline__ float comfort_mix(float p, float a, float z) {
#pragma clang fp contract(off)
    const float n = a * z;
    return p + n;
}

// kReport (calls that ask for the frame report, SynthesisArgs::report; DESIGN.md section 2, step 4, second extension): three sums over the
// row's 257 bins per emitted frame -- |X|^2, |Y|^2 and the raw mask -- formed where x[], y[] and mk[] are live, in the one order the spec
// fixes: every lane its column's chain, then a butterfly over the row's lanes.
// lane ^ 1, ^ 2 (quad_perm), then the mirrored half row and the mirrored row: after the first two steps the four lanes of a quad agree, so
// the mirrors reach "a lane of the other quad / the other half" -- the spec's Q, R, S levels.  Every lane ends with the same bits.
template <int kCtrl>
__device__ __forceinline__ float row_dpp(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), kCtrl, 0xf, 0xf, true));
}
__device__ __forceinline__ float report_row_sum(float p) {
    p = p + row_dpp<0xB1>(p);   // quad_perm [1,0,3,2]: P_c + P_(16-c) (P_0 + P_8)
    p = p + row_dpp<0x4E>(p);   // quad_perm [2,3,0,1]
    p = p + row_dpp<0x141>(p);  // row_half_mirror
    p = p + row_dpp<0x140>(p);  // row_mirror
    return p;
}
// sum of |v[k]|^2 over the row's bins: v = the lane's 16 bins k = c + 16 k2; bins 0 and 256 are real and come as dc, nyq (column 0's
// slot 0 carries both).  Products and sums stay apart, whatever the build's flags say
__device__ __forceinline__ float report_energy(const cpx (&v)[16], float dc, float nyq, int c) {
#pragma clang fp contract(off)
    const float sq = dc * dc;
    float p = __builtin_fmaf(v[0].x, v[0].x, v[0].y * v[0].y);
    p = c == 0 ? sq : p;
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) p = p + __builtin_fmaf(v[k2].x, v[k2].x, v[k2].y * v[k2].y);
    const float last = p + nyq * nyq;  // (column 0: bin 256, its 17th addend)
    p = c == 0 ? last : p;
    return report_row_sum(p);
}
__device__ __forceinline__ float report_mask_sum(const float (&m)[17], int c) {
    float p = m[0];
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) p = p + m[k2];
    const float last = p + m[16];
    p = c == 0 ? last : p;
    return report_row_sum(p);
}

// kMaskH: the mask travels as fp16 C fragments (bf16 configuration), else fp32
template <bool kRecompute, bool kMaskH, bool kMaskIn, bool kResets = false, bool kMinGain = false>
__global__ __launch_bounds__(kMaskIn ? 512 : 256, kMaskIn ? 1 : 3) void synthesis_kernel(SynthesisArgs g) {
    constexpr bool kReport = false, kLink = false, kProfile = false, kComfort = false;
#include "kns_stft_synthesis.inc"
}
// the same forms with the frame report: kernels of their own name, the same text (kns_stft_synthesis.inc) -- a call that asks for no report
// runs what it always ran
template <bool kRecompute, bool kMaskH, bool kMaskIn, bool kResets, bool kMinGain>
__global__ __launch_bounds__(kMaskIn ? 512 : 256, kMaskIn ? 1 : 3) void synthesis_report_kernel(SynthesisArgs g) {
    constexpr bool kReport = true, kLink = false, kProfile = false, kComfort = false;
#include "kns_stft_synthesis.inc"
}
// kLink (handles with channels whose link is on, SynthesisArgs::link = C; DESIGN.md section 2, eighth extension): the mask of every bin
// becomes the max over the C rows of the row's group, between the raw mask's sum and m'.  A kernel of its own name again, so the forms
// above stay the instructions they were.  The arm implies kMinGain (an all-zero gain table is exact: 0 + 1 m == m), and C is a
// wave-uniform argument, not a template parameter.  The recomputing forms exist as report forms only: without the report hipcc's
// allocation of them spilled in every variant tried, so a recomputing call that asks for no report gives the
// report's descriptor no range and the hardware drops the stores.  9 report forms + 5 plain stored-spectrum forms = 14 instantiations.
template <bool kReport, bool kRecompute, bool kMaskH, bool kMaskIn, bool kResets>
__global__ __launch_bounds__(kMaskIn ? 512 : 256, kMaskIn ? 1 : 3) void synthesis_link_kernel(SynthesisArgs g) {
    static_assert(kReport || !kRecompute, "linked, recomputed: report forms only");
    constexpr bool kMinGain = true, kLink = true, kProfile = false, kComfort = false;
#include "kns_stft_synthesis.inc"
}
// kProfile (handles with a band profile in force, SynthesisArgs::profile; DESIGN.md section 2, tenth extension): every bin's m' is held
// between the row's floor and ceiling of that bin, behind the minimum gain and in front of Y and e_out.  A kernel of its own name once more,
// so the forms above stay the instructions they were, and the arm implies kMinGain like the linked one (an all-zero gain table is exact):
// 9 forms with the report + 9 without = 18 instantiations, not twice the number there was.  There is no linked form: the engine refuses the
// combination.  The row's nine words are requested where they are consumed, four bins at a time (kns_stft_synthesis.inc): requested with the
// frame's mask and held until then, they were 36 registers more than the budget of three waves per SIMD has
template <bool kReport, bool kRecompute, bool kMaskH, bool kMaskIn, bool kResets>
__global__ __launch_bounds__(kMaskIn ? 512 : 256, kMaskIn ? 1 : 3) void synthesis_profile_kernel(SynthesisArgs g) {
    constexpr bool kMinGain = true, kLink = false, kProfile = true, kComfort = false;
#include "kns_stft_synthesis.inc"
}
// kComfort (handles on which some stream's comfort noise is on, SynthesisArgs::comfort_amp; DESIGN.md section 2, twelfth extension): behind
// m' every bin of a row whose comfort noise is on becomes Y = m' X + ((1 - m') A) z, in front of the inverse transform and of e_out.  A
// kernel of its own name once more, so the forms above stay the instructions they were.  The arm implies kMinGain and carries the profile's
// clamp (an all-zero gain table and the neutral profile are exact), so that a limit, a profile and comfort noise combine.  Nine
// instantiations, all report forms: a call that asks for no report gives the report's descriptor no range and the hardware drops the
// stores (without the report hipcc's allocation spills: some 270 bytes per lane recomputing, 12 to 20 stored).  The recomputing forms are
// built for two waves per SIMD, not three, where they still spill five registers, and fetch the frame's mask behind the forward FFT.
// There is no linked form: the engine refuses the combination.  In the stored-spectrum forms the next frame's operands are requested
// behind Y, where x[] and the amplitude words have been consumed
template <bool kReport, bool kRecompute, bool kMaskH, bool kMaskIn, bool kResets>
__global__ __launch_bounds__(kMaskIn ? 512 : 256, kMaskIn ? 1 : kRecompute ? 2 : 3) void synthesis_comfort_kernel(SynthesisArgs g) {
    static_assert(kReport, "comfort noise: report forms only");
    constexpr bool kMinGain = true, kLink = false, kProfile = true, kComfort = true;
#include "kns_stft_synthesis.inc"
}

template <bool kReport, bool kRecompute, bool kMaskH, bool kMaskIn, bool kResets, bool kMinGain, bool kLink, bool kProfile, bool kComfort>
static void launch_synthesis_form(const SynthesisArgs &a, const dim3 grid, int threads, size_t lds, hipStream_t s) {
    if constexpr (kComfort)
        hipLaunchKernelGGL((synthesis_comfort_kernel<true, kRecompute, kMaskH, kMaskIn, kResets>), grid, dim3(threads), lds, s, a);
    else if constexpr (kProfile)
        hipLaunchKernelGGL((synthesis_profile_kernel<kReport, kRecompute, kMaskH, kMaskIn, kResets>), grid, dim3(threads), lds, s, a);
    else if constexpr (kLink)
        hipLaunchKernelGGL((synthesis_link_kernel<kReport || kRecompute, kRecompute, kMaskH, kMaskIn, kResets>), grid, dim3(threads), lds, s, a);
    else if constexpr (kReport)
        hipLaunchKernelGGL((synthesis_report_kernel<kRecompute, kMaskH, kMaskIn, kResets, kMinGain>), grid, dim3(threads), lds, s, a);
    else
        hipLaunchKernelGGL((synthesis_kernel<kRecompute, kMaskH, kMaskIn, kResets, kMinGain>), grid, dim3(threads), lds, s, a);
}

// the forms of one arm (kMinGain: with or without the per-stream minimum gain; kReport: with or without the frame report); the plain arm's
// are the kernels of a handle without a limit in a call that asks for no report; kLink: the linked kernels, which carry the gain; kProfile:
// the profile kernels, which carry it too; kComfort: the comfort kernels, which carry the gain and the profile
template <bool kMinGain, bool kReport, bool kLink = false, bool kProfile = false, bool kComfort = false>
static void launch_synthesis_arm(const SynthesisArgs &a, const dim3 grid, size_t lds, hipStream_t s) {
    if (a.resets) {  // (calls with per-frame stream resets: the reset arm; the engine does not put the mask head inside then)
        if (a.recompute && a.mask_fp16)
            launch_synthesis_form<kReport, true, true, false, true, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
        else if (a.recompute)
            launch_synthesis_form<kReport, true, false, false, true, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
        else if (a.mask_fp16)
            launch_synthesis_form<kReport, false, true, false, true, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
        else
            launch_synthesis_form<kReport, false, false, false, true, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
    } else if (a.mask_w && !a.recompute && a.mask_fp16 && a.T == 1)
        launch_synthesis_form<kReport, false, true, true, false, kMinGain, kLink, kProfile, kComfort>(a, grid, 512, lds + kMaskTiles * 512, s);
    else if (a.recompute && a.mask_fp16)
        launch_synthesis_form<kReport, true, true, false, false, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
    else if (a.recompute)
        launch_synthesis_form<kReport, true, false, false, false, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
    else if (a.mask_fp16)
        launch_synthesis_form<kReport, false, true, false, false, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
    else
        launch_synthesis_form<kReport, false, false, false, false, kMinGain, kLink, kProfile, kComfort>(a, grid, 256, lds, s);
}

void launch_synthesis(const SynthesisArgs &a, hipStream_t s) {
    const size_t lds = kOffStftEnd + KNS_STFT_LDS_PAD;
    const dim3 grid(a.Bpad / 16, (a.T + a.seg - 1) / a.seg);
#if KNS_STFT_LDS_PAD
    (void) hipFuncSetAttribute((const void *) synthesis_kernel<true, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
    (void) hipFuncSetAttribute((const void *) synthesis_report_kernel<true, true, false, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
#endif
    if (a.comfort_amp)  // (the engine hands such a launch the gain table and the profile, neutral where none is in force, and no link)
        a.report ? launch_synthesis_arm<true, true, false, true, true>(a, grid, lds, s) : launch_synthesis_arm<true, false, false, true, true>(a, grid, lds, s);
    else if (a.profile)  // (the engine hands a profiled launch the gain table, all zero where no limit is in force, and no link)
        a.report ? launch_synthesis_arm<true, true, false, true>(a, grid, lds, s) : launch_synthesis_arm<true, false, false, true>(a, grid, lds, s);
    else if (a.link)  // (the engine hands a linked launch the gain table, all zero where no limit is in force)
        a.report ? launch_synthesis_arm<true, true, true>(a, grid, lds, s) : launch_synthesis_arm<true, false, true>(a, grid, lds, s);
    else if (a.report)
        a.min_gain ? launch_synthesis_arm<true, true>(a, grid, lds, s) : launch_synthesis_arm<false, true>(a, grid, lds, s);
    else if (a.min_gain)
        launch_synthesis_arm<true, false>(a, grid, lds, s);
    else
        launch_synthesis_arm<false, false>(a, grid, lds, s);
}

// ------------------------------------------------------------------------------------------------ reset

__global__ void reset_kernel(ResetArgs g) {
    // one workgroup per stream: history, overlap-add tail, and this stream's row of the 8 hidden-state tiles
    const int b = blockIdx.x, tid = threadIdx.x;
    if (g.mask && !g.mask[b]) return;
    g.hist[(size_t) b * kFrame + tid] = 0;
    g.hist2[(size_t) b * kFrame + tid] = 0;
    g.tail[(size_t) b * kFrame + tid] = 0.0f;
    g.tail2[(size_t) b * kFrame + tid] = 0.0f;
    const int mtiles = g.Bpad >> 4, mt = b >> 4, row = b & 15;
    for (int i = tid; i < kGruLayers * kUnitTiles * 16; i += 256) {
        const int col = i & 15, u = (i >> 4) % kUnitTiles, layer = (i >> 4) / kUnitTiles;
        const size_t idx = (((size_t) layer * mtiles + mt) * kUnitTiles + u) * 256 + cpack_off(row, col);
        g.hstate[idx] = 0.0f;
        g.hstate2[idx] = 0.0f;
    }
    // front-end context: this stream's row of every k-block of every remembered frame = the feature of a silent frame (in
    // an A-packed block a row is the four 16-byte words of lanes row, row + 16, row + 32, row + 48)
    for (int i = tid; i < g.fhist_frames * g.nbf * 4; i += 256) {
        const int q = i & 3, kb = (i >> 2) % g.nbf, f = (i >> 2) / g.nbf;
        const size_t word = (size_t) kb * 64 + row + 16 * q;
        ((uint4 *) g.fhist)[((size_t) f * mtiles + mt) * g.nbf * 64 + word] = ((const uint4 *) g.silent)[word];
    }
}

// ---- completion word of a one-frame graph replay: the last node of the captured frame.  Counts the replays on the device and
// publishes the count to a word in page-locked host memory with a system-scope release: a host that sees the count sees the frame's
// output (written to host memory by the synthesis kernel, complete at the kernel boundary before this node runs).
__global__ void frame_done_kernel(unsigned *counter, unsigned *host_word) {
    const unsigned v = *counter + 1u;
    *counter = v;
    __hip_atomic_store(host_word, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

void launch_frame_done(unsigned *counter, unsigned *host_word, hipStream_t s) {
    hipLaunchKernelGGL(frame_done_kernel, dim3(1), dim3(1), 0, s, counter, host_word);
}

void launch_reset(const ResetArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(reset_kernel, dim3(a.Bpad), dim3(256), 0, s, a);
}

}  // namespace kns
