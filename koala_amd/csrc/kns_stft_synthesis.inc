// kns_stft_synthesis.inc -- the body of the synthesis kernels of kns_stft.hip, included once per kernel template: synthesis_kernel
// (kReport = false) and synthesis_report_kernel (kReport = true).  Text, not a function: the kernels of a call without a report must be the
// instructions they were before the report existed (tools/asm_same.py), and a body inlined into two kernels through a function call was
// not -- hipcc ordered and allocated it differently.  In scope: g (SynthesisArgs), kRecompute, kMaskH, kMaskIn, kResets, kMinGain, kReport,
// kLink, kProfile, kComfort.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    static_assert(!kMaskIn || (kMaskH && !kRecompute), "mask head inside: bf16, stored spectrum");
    static_assert(!kMaskIn || !kResets, "resets: multi-frame form only");

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (kMaskIn && wave >= 4) {
        typedef PBF16 P;
        typedef P::frag_t frag_t;
        constexpr int NB = P::NBH, kPer = (kMaskTiles + 3) / 4;
        const int gw = wave - 4, colq = lane & 15;
        frag_t a[NB], w[kPer][NB];
        float bias[kPer];
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) a[kb] = ((const frag_t *) g.mask_h)[((size_t) blockIdx.x * NB + kb) * 64 + lane];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {  // n-tiles gw, gw + 4, ...; a slot past the last tile repeats it (same words, same values)
            const int nt = gw + 4 * q < kMaskTiles ? gw + 4 * q : kMaskTiles - 1;
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) w[q][kb] = ((const frag_t *) g.mask_w)[((size_t) nt * NB + kb) * 64 + lane];
            bias[q] = g.mask_b[nt * 16 + colq];
        }
        __builtin_amdgcn_sched_barrier(0);  // every request before the first use (the scheduler would sink the loads to save registers)
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int nt = gw + 4 * q < kMaskTiles ? gw + 4 * q : kMaskTiles - 1;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) acc = P::mma(a[kb], w[q][kb], acc);
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = head_sigmoid<P>(acc[i] + bias[q]);
            ((f16x4 *) (smem + kOffStftEnd))[nt * 64 + lane] = __builtin_convertvector(v, f16x4);
        }
        __syncthreads();
        return;
    }
    const int c = fft_column(lane), q = lane >> 4, row = wave * 4 + q;
    const int mt = blockIdx.x, mtiles = g.Bpad >> 4;
    const int t0 = blockIdx.y * g.seg, t1 = min(g.T, t0 + g.seg);
    const int tb = t0 > 0 ? t0 - 1 : 0;
    const int b = mt * 16 + row;
    const bool valid = b < g.B;
    const size_t row_len = (size_t) (g.pitch ? g.pitch : g.T) * kFrame;
    const int16_t *pcm_row = g.pcm + (size_t) (valid ? b : g.B - 1) * row_len;  // (ragged tile: see analysis_kernel)
    // this row's minimum gain and its complement (the table has Bpad entries: rows past the last stream read their own, a zero)
    float mg = 0.0f, mu = 1.0f;
    if (kMinGain) {
        mg = g.min_gain[b];
        mu = 1.0f - mg;
    }
    // kProfile: this lane's words of its row of the band-profile table (kns_kernels.h, profile_index: floors of its 16 bins, their ceilings,
    // and the Nyquist pair behind the row's 16 lanes; the table has Bpad rows like the gains').  Nine 16-byte loads per frame through one
    // wave-uniform descriptor over the wave's four rows -- what stays live across the frame loop is one offset register, not the table
    const unsigned pf_off = (unsigned) q * (unsigned) (kProfileRow * 4) + (unsigned) c * 128u;
    auto profile_word = [&](unsigned byte_off, unsigned imm) {
        const __amdgpu_buffer_rsrc_t pr = make_rsrc(g.profile + (size_t) (mt * 16 + wave * 4) * kProfileRow, 4u * kProfileRow * 4u);
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(pr, byte_off, imm, 0));
    };
    // kComfort: the row's setting and the frame's counter value are fetched where they are used, through wave-uniform descriptors over the
    // wave's four rows -- kept across the frame loop they were registers the recomputing forms do not have; the lane's words of the amplitude
    // table (kns_kernels.h, comfort_index: four words of its 16 bins and the Nyquist word behind the row's 16 lanes) like the profile's
    const unsigned cf_off = (unsigned) q * (unsigned) (kComfortRow * 4) + (unsigned) c * 64u;
    auto comfort_word = [&](unsigned byte_off, unsigned imm) {
        const __amdgpu_buffer_rsrc_t cr = make_rsrc(g.comfort_amp + (size_t) (mt * 16 + wave * 4) * kComfortRow, 4u * kComfortRow * 4u);
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(cr, byte_off, imm, 0));
    };

    int prev[8], cur[8], nxt[8];
    if (kRecompute) {
        load_frame(prev, tb == 0 && !g.prev_in_pcm ? g.hist_in + (size_t) b * kFrame : pcm_row + ((ptrdiff_t) tb - 1) * kFrame, c);
        load_frame(cur, pcm_row + (size_t) tb * kFrame, c);
    }
    // overlap-add tail of this lane's points n = c + 16 k2, k2 = 8..15 (samples 2n, 2n + 1 of the block's second half)
    cpx tl[8];
    {
        const float2 *tp = (const float2 *) (g.tail_in + (size_t) b * kFrame);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float2 v = tp[c + 16 * j];
            tl[j] = cpx{v.x, v.y};
        }
    }
    // mask element (row, k): C-packed tile k / 16, lane (row >> 2) * 16 + (k & 15), value row & 3 -- for a fixed k2 the
    // wave reads one contiguous 1 KiB tile
    const unsigned mlane = ((unsigned) (wave * 16 + c) * 4u + (unsigned) q) * 4u;
    float mk[17], mkn[17];
    auto mask_fetch = [&](float (&m)[17], int t) {
        if (kMaskIn) {  // this workgroup's tile, computed by waves 4..7 into LDS
            const _Float16 *ml = (const _Float16 *) (smem + kOffStftEnd);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) m[k2] = (float) ml[k2 * 256 + (mlane >> 2)];
            m[16] = (float) ml[16 * 256 + (wave * 16) * 4 + q];
            return;
        }
        if (kMaskH) {  // fp16 tiles of 512 B; the conversion to fp32 is exact
            const __amdgpu_buffer_rsrc_t mr =
                make_rsrc((const char *) g.mask + ((size_t) t * mtiles + mt) * kMaskTiles * 512, kMaskTiles * 512);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2)
                m[k2] = (float) __builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(mr, mlane >> 1, k2 * 512u, 0));
            m[16] = (float) __builtin_bit_cast(
                _Float16, __builtin_amdgcn_raw_buffer_load_b16(mr, ((unsigned) (wave * 16) * 4u + (unsigned) q) * 2u, 16 * 512u, 0));
            return;
        }
        const __amdgpu_buffer_rsrc_t mr = make_rsrc(g.mask + ((size_t) t * mtiles + mt) * kMaskTiles * 256, kMaskTiles * 1024);
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2)
            m[k2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mr, mlane, k2 * 1024u, 0));
        m[16] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mr, ((unsigned) (wave * 16) * 4u + (unsigned) q) * 4u, 16 * 1024u, 0));
    };
    // kLink: the 17 mask values of a partner row of this lane's group, frame t -- the fetch above for another row of the tile (elem: the
    // partner's element of tiles 0..15, (row' >> 2) * 64 + c * 4 + (row' & 3); elem_n: of tile 16's column 0).  The words are the ones the
    // wave pair's lanes read their own values from
    auto mask_partner = [&](float (&m)[17], int t, unsigned elem, unsigned elem_n) {
        if (kMaskIn) {
            const _Float16 *ml = (const _Float16 *) (smem + kOffStftEnd);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) m[k2] = (float) ml[k2 * 256 + elem];
            m[16] = (float) ml[16 * 256 + elem_n];
            return;
        }
        if (kMaskH) {
            const __amdgpu_buffer_rsrc_t mr =
                make_rsrc((const char *) g.mask + ((size_t) t * mtiles + mt) * kMaskTiles * 512, kMaskTiles * 512);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2)
                m[k2] = (float) __builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(mr, elem * 2u, k2 * 512u, 0));
            m[16] = (float) __builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(mr, elem_n * 2u, 16 * 512u, 0));
            return;
        }
        const __amdgpu_buffer_rsrc_t mr = make_rsrc(g.mask + ((size_t) t * mtiles + mt) * kMaskTiles * 256, kMaskTiles * 1024);
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) m[k2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mr, elem * 4u, k2 * 1024u, 0));
        m[16] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mr, elem_n * 4u, 16 * 1024u, 0));
    };
    cpx xs[16], xsn[16];
    auto spec_fetch = [&](cpx (&dst)[16], int t) {
        const f32x4 *spec = (const f32x4 *) g.spec + ((size_t) t * g.Bpad + b) * 128;
#pragma unroll
        for (int k2 = 0; k2 < 16; k2 += 2) {
            const f32x4 v = spec[(k2 >> 1) * 16 + c];
            dst[k2] = cpx{v[0], v[1]};
            dst[k2 + 1] = cpx{v[2], v[3]};
        }
    };
    // stored spectrum: the first frame's operands are requested before the tables are waited for (one memory round trip in front
    // of the first FFT, not two)
    if (!kRecompute) {
        if (!kMaskIn) mask_fetch(mk, tb);
        spec_fetch(xs, tb);
    }
    StftTables tbl;
    stft_request_tables(tbl, g.twiddle, g.window, tid);
    stft_store_tables<true>(tbl, smem, tid);
    __syncthreads();
    char *xw;
    const char *xr, *twl_c;
    fft_lane_bases(smem + kOffXbuf + wave * kFftWaveBytes, smem + kOffTwl, lane, &xw, &xr, &twl_c);
    const char *tw_c = smem + kOffTw + c * 8, *win_c = smem + kOffWin + c * 8, *wins_c = smem + kOffWinS + c * 8;
    if (kMaskIn) mask_fetch(mk, tb);  // (complete since the barrier)

    for (int t = tb; t < t1; ++t) {
        const bool emit = t >= t0;
        const int tn = t + 1 < t1 ? t + 1 : t;
        // recompute: the mask is not needed before the first FFT and the spectrum are through (~700 instructions), so it is
        // requested here without a second register set; stored spectrum: mask and spectrum of the next frame in flight
        // (kProfile, stored spectrum: the next frame's operands are requested behind m', where the profile's words have been consumed -- with
        // both in flight at once the forms did not fit the registers of three waves per SIMD; the inverse FFT still lies in front of their use)
        // (kComfort, recomputed: behind the forward FFT -- held across it, the 17 values were registers the forms do not have)
        if (kRecompute) {
            if (!kComfort) mask_fetch(mk, t);
        } else if (!kProfile)
            mask_fetch(mkn, tn);
        if (kResets) {
            const unsigned rm = reset_rows(g.resets, g.rs_pitch, mt, g.rs_t0 + t);
            if (rm) {
                const bool r = (rm >> row) & 1u;
#pragma unroll
                for (int j = 0; j < 8; ++j) tl[j] = r ? cpx{0.0f, 0.0f} : tl[j];
                if (kRecompute) {
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) prev[jj] = r ? 0 : prev[jj];
                }
            }
        }
        cpx x[16];
        if (kRecompute) {
            load_frame(nxt, pcm_row + (size_t) tn * kFrame, c);
            cpx v[16];
            window_block(v, prev, cur, win_c);
            fft256_rows(v, twl_c, xw, xr);
            real_spectrum(v, x, tw_c, c);
            if (kComfort) mask_fetch(mk, t);
        } else {
            if (!kProfile) spec_fetch(xsn, tn);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) x[k2] = xs[k2];
        }
        // Y = mask . X; bin 0 holds DC and Nyquist (both real): its slot travels as {m[0] X[0], m[256] X[256]} and is taken
        // apart again below
        // (kMinGain: on m' -- formed here, where the frame's mask is first used, so the request above stays in flight as long as before)
        // (kReport: e_in from X, mask_sum from the network's mask m -- before m' takes its place.  Each value of the frame's report row leaves
        // where it is formed: held until the samples are stored, the three of them were three registers too many in the recomputing
        // reset forms.  One dword per store from the row's first lane, every lane holding the same bits; the other lanes, rows past the last
        // stream and the replayed frame fall outside the wave-uniform descriptor's range, like the samples below)
        // (the descriptor is rebuilt from scalars at either place, like the samples' below: kept in a variable across the frame it ended up in
        // vector registers, and hipcc wrapped every store in a loop over the distinct descriptors)
        auto report_rsrc = [&]() {
            const int row0 = mt * 16 + wave * 4;
            const int rows_ok = row0 < g.B ? min(4, g.B - row0) : 0;
            const unsigned rep_row = (unsigned) (g.pitch ? g.pitch : g.T) * 16u;  // (bytes between two streams' rows: at most 2^20 frames)
            // (kLink, kComfort: the recomputing linked and comfort kernels are report forms only; a call that asks for no report has no rows in range)
            const unsigned rspan = emit && rows_ok && (!(kLink || kComfort) || g.report) ? (unsigned) (rows_ok - 1) * rep_row + 16u : 0u;
            // (wave-uniform by construction; said explicitly, since hipcc otherwise keeps the loop-invariant product in a vector register)
            return make_rsrc((const char *) g.report + (size_t) row0 * rep_row + (size_t) t * 16, (unsigned) __builtin_amdgcn_readfirstlane((int) rspan));
        };
        const unsigned roff = c == 0 ? (unsigned) q * (unsigned) ((g.pitch ? g.pitch : g.T) * 16) : 0x7ffffff0u;
        if (kReport) {
            const __amdgpu_buffer_rsrc_t ro = report_rsrc();
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, report_energy(x, x[0].x, x[0].y, c)), ro, roff, 0u, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, report_mask_sum(mk, c)), ro, roff, 8u, 0);
            __builtin_amdgcn_raw_buffer_store_b32(0, ro, roff, 12u, 0);
        }
        // (kLink: m becomes the max over the rows of the lane's group, rows (row & -C) .. + C - 1 of the tile = row ^ j, j = 1 .. C - 1.  Here,
        // behind the raw mask's sum and in front of m', for the reason given at kMinGain.  C is wave-uniform: a scalar loop over the partners,
        // one partner's 17 values at a time, so the arm costs 17 registers whatever C is.  An element index is wave * 64 + c * 4 + q: the
        // partner's differs from the lane's own in the wave bit j >> 2 and the value bits j & 3)
        if (kLink) {
            for (int j = 1; j < g.link; ++j) {
                const unsigned flip = (unsigned) (((j >> 2) << 6) | (j & 3));
                float pm[17];
                mask_partner(pm, t, (mlane >> 2) ^ flip, ((unsigned) (wave * 16) * 4u + (unsigned) q) ^ flip);
#pragma unroll
                for (int k2 = 0; k2 < 17; ++k2) mk[k2] = link_max(mk[k2], pm[k2]);
            }
        }
        if (kMinGain) {
#pragma unroll
            for (int k2 = 0; k2 < 17; ++k2) mk[k2] = min_gain_mask(mg, mu, mk[k2]);
        }
        // (kProfile: m' = min(ceil, max(floor, m')), max first -- behind the gain, in front of Y and of e_out; exact)
        if (kProfile) {
            // four bins at a time -- a floor word, a ceiling word -- with the next four's words in flight: two groups live, never all nine
            // words (left to itself hipcc requests all of them first, 36 registers that three waves per SIMD do not have)
            f32x4 pfl = profile_word(pf_off, 0u), pce = profile_word(pf_off, 64u);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 nfl = profile_word(i < 3 ? pf_off : (unsigned) q * (unsigned) (kProfileRow * 4), i < 3 ? 16u * (i + 1) : 2048u);
                f32x4 nce = nfl;
                if (i < 3) nce = profile_word(pf_off, 64u + 16u * (i + 1));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) mk[4 * i + j] = profile_clamp(pfl[j], pce[j], mk[4 * i + j]);
                __builtin_amdgcn_sched_barrier(0);
                pfl = nfl, pce = nce;
            }
            mk[16] = profile_clamp(pfl[0], pfl[1], mk[16]);  // (the row's last word: floor[256], ceil[256])
            if (!kRecompute && !kComfort) {
                mask_fetch(mkn, tn);
                spec_fetch(xsn, tn);
            }
        }
        cpx y[16];
        float y_nyq = 0.0f;  // (kComfort, column 0: Y[256])
        if (kComfort) {
            // Y = m' X + ((1 - m') A) z, z the hash of (seed, n, k): behind m', in front of e_out.  Four bins at a time, one word of the
            // amplitude row each with the next in flight, like the profile's words; a row whose comfort noise is off keeps m' X, bit for bit
            const int row0c = mt * 16 + wave * 4;
            const unsigned npitch = (unsigned) (g.pitch ? g.pitch : g.T);
            const __amdgpu_buffer_rsrc_t sr = make_rsrc(g.comfort_set + row0c, 4u * 8u);
            const __amdgpu_buffer_rsrc_t nr = make_rsrc(g.comfort_n + (size_t) row0c * npitch + t, (3u * npitch + 1u) * 4u);
            const int cn_on = __builtin_amdgcn_raw_buffer_load_b32(sr, (unsigned) q * 8u, 0u, 0);
            const unsigned cn_seed = (unsigned) __builtin_amdgcn_raw_buffer_load_b32(sr, (unsigned) q * 8u, 4u, 0);
            const unsigned cn_n = (unsigned) __builtin_amdgcn_raw_buffer_load_b32(nr, (unsigned) q * npitch * 4u, 0u, 0);
            const unsigned base = cn_seed ^ (cn_n * 0x9E3779B9u);
            f32x4 am = comfort_word(cf_off, 0u);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 nam = comfort_word(i < 3 ? cf_off : (unsigned) q * (unsigned) (kComfortRow * 4), i < 3 ? 16u * (i + 1) : 1024u);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k2 = 4 * i + j;
                    const unsigned v = comfort_hash(base, (unsigned) (c + 16 * k2));
                    const float zi = (k2 == 0 && c == 0) ? 0.0f : comfort_variate(v >> 16);
                    const float a = comfort_amplitude(mk[k2], am[j]);
                    const float pr = mk[k2] * x[k2].x, pi = mk[k2] * x[k2].y;
                    y[k2] = cpx{cn_on ? comfort_mix(pr, a, comfort_variate(v & 0xffffu)) : pr, cn_on ? comfort_mix(pi, a, zi) : pi};
                }
                __builtin_amdgcn_sched_barrier(0);
                am = nam;
            }
            {  // (the row's last word: A[256]; bin 256 is real and travels in bin 0's imaginary slot)
                const unsigned v = comfort_hash(base, 256u);
                const float pn = mk[16] * x[0].y;
                y_nyq = cn_on ? comfort_mix(pn, comfort_amplitude(mk[16], am[0]), comfort_variate(v & 0xffffu)) : pn;
            }
            if (!kRecompute) {
                mask_fetch(mkn, tn);
                spec_fetch(xsn, tn);
            }
        } else {
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) y[k2] = cpx{mk[k2] * x[k2].x, mk[k2] * x[k2].y};
        }
        if (kReport)  // (column 0: Y[0] = m'[0] X0, Y[256] = m'[256] X256)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, report_energy(y, y[0].x, kComfort ? y_nyq : mk[16] * x[0].y, c)), report_rsrc(), roff, 4u, 0);
        cpx yp[16];
        fft_partner(y, yp, c);
        cpx v[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            cpx yk = y[k2], yq = yp[k2];  // Y[k], Y[256 - k]
            if (k2 == 0 && c == 0) {
                yk = cpx{kComfort ? y[0].x : mk[0] * x[0].x, 0.0f};
                yq = cpx{kComfort ? y_nyq : mk[16] * x[0].y, 0.0f};
            }
            const float2 w = *(const float2 *) (tw_c + k2 * 128);
            // e = Y[k] + conj(Y[256 - k]), d = Y[k] - conj(Y[256 - k]), o = conj(W^k) d
            const cpx e = {yk.x + yq.x, yk.y - yq.y}, d = {yk.x - yq.x, yk.y + yq.y};
            const cpx o = cmul(d, cpx{w.x, -w.y});
            // Z' = E + i O (both carry the factor 1/2); fed to the forward FFT with re/im swapped = inverse FFT
            const float zr = 0.5f * (e.x - o.y), zi = 0.5f * (e.y + o.x);
            v[k2] = cpx{zi, zr};
        }
        fft256_rows(v, twl_c, xw, xr);
        int packed[8];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            const float2 w = *(const float2 *) (wins_c + k2 * 128);  // window[2n] / 256, window[2n + 1] / 256, n = c + 16 k2
            // swapped output: re <-> im; = (v / 256) window: the table carries the 2^-8
            const float y0 = v[k2].y * w.x, y1 = v[k2].x * w.y;
            if (k2 < 8) {
                float a0 = (tl[k2].x + y0) * 32768.0f, a1 = (tl[k2].y + y1) * 32768.0f;
                a0 = __builtin_fminf(__builtin_fmaxf(__builtin_roundf(a0), -32768.0f), 32767.0f);
                a1 = __builtin_fminf(__builtin_fmaxf(__builtin_roundf(a1), -32768.0f), 32767.0f);
                packed[k2] = ((int) a0 & 0xffff) | ((int) a1 << 16);
            } else {
                v[k2] = cpx{y0, y1};
            }
        }
#pragma unroll
        for (int k2 = 8; k2 < 16; ++k2) tl[k2 - 8] = v[k2];
        {
            // one wave-uniform descriptor over the wave's four stream rows of this frame (a per-lane base would make hipcc
            // wrap every store in a loop over the distinct descriptors); rows that must not be written -- the replayed
            // frame, streams past the last one -- fall outside the descriptor's range and are dropped by the hardware
            const int row0 = mt * 16 + wave * 4;
            const int rows_ok = row0 < g.B ? min(4, g.B - row0) : 0;
            const unsigned span = emit && rows_ok ? (unsigned) ((size_t) (rows_ok - 1) * row_len * 2 + kFrame * 2) : 0u;
            const __amdgpu_buffer_rsrc_t o = make_rsrc(g.out + (size_t) row0 * row_len + (size_t) t * kFrame, span);
            const unsigned voff = (unsigned) q * (unsigned) (row_len * 2) + (unsigned) c * 4u;
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) __builtin_amdgcn_raw_buffer_store_b32(packed[k2], o, voff, 64u * k2, 0);
        }
        if (kRecompute) {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                prev[jj] = cur[jj];
                cur[jj] = nxt[jj];
            }
        } else {
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) xs[k2] = xsn[k2];
        }
        if (!kRecompute) {
#pragma unroll
            for (int k2 = 0; k2 < 17; ++k2) mk[k2] = mkn[k2];
        }
    }
    if (t1 == g.T) {
        float2 *tp = (float2 *) (g.tail_out + (size_t) b * kFrame);
#pragma unroll
        for (int j = 0; j < 8; ++j) tp[c + 16 * j] = float2{tl[j].x, tl[j].y};
    }
