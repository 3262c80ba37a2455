// The format kernels' REAL source over the matrices the engine gives them: the dense matrix of a frame call (one row of B T F elements), the
// whole rows of a packet call on the way in, and its counted rows on the way out -- every format, both directions, the caller's side and the
// int16 side each starting at several byte offsets.  Every buffer is an allocation of exactly its size (the sanitizer's red zones are the
// guard behind it) filled with a pattern: the bytes in front of the base and every element at and past counts[b] must keep it.  The
// codecs are restated here with loops instead of a count of leading zeros.
using namespace kns;

static int bit_length(int v) { int n = 0; while (v) ++n, v >>= 1; return n; }
static int ref_dec(int fmt, const uint8_t *p) {
    if (fmt == kFmtF32) {
        float x; memcpy(&x, p, 4);
        if (std::isnan(x)) return 0;
        const double y = (double) x * 32768.0;  // (exact in double too)
        if (y >= 32767.0) return 32767;
        if (y <= -32768.0) return -32768;
        const double r = std::floor(std::fabs(y) + 0.5);
        return (int) (y < 0 ? -r : r);
    }
    const int b = *p;
    if (fmt == kFmtUlaw) {
        const int u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84;
        return (u & 0x80) ? -mag : mag;
    }
    const int a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
    return (a & 0x80) ? mag : -mag;
}
static void ref_enc(int fmt, int s, uint8_t *p) {
    if (fmt == kFmtF32) { const float f = (float) s / 32768.0f; memcpy(p, &f, 4); return; }
    if (fmt == kFmtUlaw) {
        const int sign = s < 0 ? 0x80 : 0, mag = std::min(std::abs(s), 32635) + 0x84, e = bit_length(mag) - 8, m = (mag >> (e + 3)) & 15;
        *p = (uint8_t) (~(sign | e << 4 | m) & 0xFF);
        return;
    }
    const int sign = s >= 0 ? 0x80 : 0, mag = s >= 0 ? s : ~s, e = mag < 256 ? 0 : bit_length(mag) - 8;
    const int m = e == 0 ? (mag >> 4) & 15 : (mag >> (e + 3)) & 15;
    *p = (uint8_t) ((sign | e << 4 | m) ^ 0x55);
}

template <class K> static void launch(K kernel, const FormatArgs &a, int fmt) {
    const long long bpr = (a.n / fmt_group(fmt) + 2 + 255) / 256;
    for (long long b = 0; b < bpr * a.rows; ++b)
        for (unsigned t = 0; t < 256; ++t) { blockIdx.x = (unsigned) b, threadIdx.x = t; kernel(a); }
}
static void run_kernel(int fmt, bool in, const FormatArgs &a) {
    if (fmt == kFmtF32) in ? launch(format_in_kernel<kFmtF32>, a, fmt) : launch(format_out_kernel<kFmtF32>, a, fmt);
    else if (fmt == kFmtUlaw) in ? launch(format_in_kernel<kFmtUlaw>, a, fmt) : launch(format_out_kernel<kFmtUlaw>, a, fmt);
    else in ? launch(format_in_kernel<kFmtAlaw>, a, fmt) : launch(format_out_kernel<kFmtAlaw>, a, fmt);
}

static const float kEdges[] = {0.0f, -0.0f, 1.0f, -1.0f, 1.0f - 1.0f / 65536, -(1.0f - 1.0f / 65536), 0.5f / 32768, -0.5f / 32768, 1.5f / 32768,
                               -2.5f / 32768, 1e30f, -1e30f, INFINITY, -INFINITY, NAN, 1e-40f, 32766.5f / 32768, -32767.5f / 32768, 0.49999997f / 32768};
static unsigned g_seed = 12345;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// one matrix [rows][n] through one kernel; counts: per row, or nullptr.  Returns the number of elements checked, -1 on a mismatch.
static long long one_case(int fmt, bool in, int rows, long long n, const std::vector<int32_t> *counts, int off_fmt, int off_s16) {
    const int eb = fmt_bytes(fmt), sb = in ? eb : 2, db = in ? 2 : eb, soff = in ? off_fmt : off_s16, doff = in ? off_s16 : off_fmt;
    const size_t total = (size_t) rows * n;
    uint8_t *sblock = (uint8_t *) malloc(soff + total * sb), *dblock = (uint8_t *) malloc(doff + total * db);
    if (((uintptr_t) sblock | (uintptr_t) dblock) & 15) { printf("allocator gave an unaligned block\n"); return -1; }
    uint8_t *src = sblock + soff, *dst = dblock + doff;
    memset(sblock, 0x3C, soff), memset(dblock, 0xA5, doff + total * db);
    for (size_t i = 0; i < total; ++i) {
        if (!in) { const int16_t s = i % 97 == 0 ? (int16_t) -32768 : i % 89 == 0 ? (int16_t) 32767 : (int16_t) (rnd() & 0xFFFF); memcpy(src + 2 * i, &s, 2); }
        else if (fmt != kFmtF32) src[i] = (uint8_t) (i < 256 ? i : rnd());
        else {
            float f = i < sizeof(kEdges) / 4 ? kEdges[i] : (rnd() & 3) ? (float) (int16_t) (rnd() & 0xFFFF) / 32768.0f : ((float) (rnd() & 0xFFFFF) / 524288.0f - 1.0f) * 1.1f;
            memcpy(src + 4 * i, &f, 4);
        }
    }
    FormatArgs a{src, dst, counts ? counts->data() : nullptr, n, rows};
    run_kernel(fmt, in, a);
    long long checked = 0;
    for (int k = 0; k < doff; ++k) if (dblock[k] != 0xA5) { printf("wrote in front of the base\n"); return -1; }
    for (int b = 0; b < rows; ++b) {
        const long long c = counts ? (*counts)[b] : n;
        for (long long i = 0; i < n; ++i) {
            const size_t at = (size_t) b * n + i;
            uint8_t want[4] = {0xA5, 0xA5, 0xA5, 0xA5};
            if (i < c) {
                if (in) { const int16_t s = (int16_t) ref_dec(fmt, src + at * sb); memcpy(want, &s, 2); }
                else { int16_t s; memcpy(&s, src + at * 2, 2); ref_enc(fmt, s, want); }
                ++checked;
            }
            if (memcmp(want, dst + at * db, db)) {
                printf("fmt %d in %d rows %d n %lld offsets %d %d: row %d element %lld (count %lld) is wrong\n", fmt, (int) in, rows, n, off_fmt, off_s16, b, i, c);
                return -1;
            }
        }
    }
    free(sblock), free(dblock);
    return checked;
}

int main() {
    long long checked = 0;
    int cases = 0;
    for (int fmt = kFmtF32; fmt <= kFmtAlaw; ++fmt) {
        const int offs8[] = {0, 1, 15}, offs32[] = {0, 4, 12}, offs16[] = {0, 2};
        for (int in = 0; in < 2; ++in)
            for (int fo = 0; fo < 3; ++fo)
                for (int so = 0; so < 2; ++so) {
                    const int off_fmt = fmt == kFmtF32 ? offs32[fo] : offs8[fo], off_s16 = offs16[so];
                    for (int TF : {128, 256, 768}) {  // a frame call: B = 3, the dense matrix as one row
                        const long long r = one_case(fmt, in, 1, 3LL * TF, nullptr, off_fmt, off_s16);
                        if (r < 0) return 1;
                        checked += r, ++cases;
                    }
                    for (int maxs : {1, 80, 701}) {  // a packet call: whole rows in, counted rows out
                        const int B = 6;
                        const std::vector<int32_t> counts{0, 1, maxs, maxs > 2 ? maxs / 2 | 1 : 1, maxs > 40 ? 37 : maxs, maxs > 3 ? maxs - 1 : 0};
                        const long long r = in ? one_case(fmt, true, 1, (long long) B * maxs, nullptr, off_fmt, off_s16)
                                               : one_case(fmt, false, B, maxs, &counts, off_fmt, off_s16);
                        if (r < 0) return 1;
                        checked += r, ++cases;
                    }
                }
    }
    printf("format kernels ok: %d cases, %lld elements\n", cases, checked);
    return 0;
}
