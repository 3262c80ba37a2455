// kns_kernels.h -- launch interface of the gfx950 kernels (kns_stft.hip, kns_gemm.hip, kns_gru.hip).  Host code only sees PODs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kns_layout.h"

namespace kns {

// A kernel that asks for more dynamic LDS than the default limit needs the attribute once PER DEVICE (a process may hold
// engines on several GPUs): remembered per kernel instantiation and device.
template <class Kernel>
inline void allow_dynamic_lds(Kernel kernel, size_t bytes) {
    static unsigned long long done = 0;  // bit d: set on device d (launches of one engine come from one thread at a time)
    int dev = 0;
    (void) hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done & bit) return;
    (void) hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
    done |= bit;
}


// Developer switches (kernel A/B selection, tuning knobs, probing modes) exist only in the -DKNS_DEV build
// (lib/libpv_koala_dev.so, used by tests/ and tools/); the product library reads none of them.
#ifdef KNS_DEV
inline const char *dev_env(const char *name) { return getenv(name); }
#else
inline const char *dev_env(const char *) { return nullptr; }
#endif
// kernel-family overrides carried in the launch arguments (set by the engine from its developer switches; 0 in the product)
enum DevVariant { kDevGruStream = 1, kDevGemmGeneric = 2, kDevGemmNoWsr = 4 };

// ---- analysis: int16 frames -> spectrum + normalised log-power features (SURVEY 8a rows a2+a3)
struct AnalysisArgs {
    const int16_t *pcm;       // [B][T*256] row-major (caller layout)
    const int16_t *hist_in;   // [Bpad][256] last frame of the previous call
    int16_t *hist_out;        // [Bpad][256] last frame of this call
    const float *window;      // [512]
    const float *twiddle;     // [512][2] exp(-2 pi i k / 512)
    const float *mean;        // [257]
    const float *scale;       // [257]
    float *spec;              // [T][Bpad][256][2] packed half spectrum (bin 0 = {X0.re, X256.re}); bin k = c + 16 k2 sits at
                              // complex slot ((k2 >> 1) * 16 + c) * 2 + (k2 & 1): the STFT kernels' lane order
    void *feat;               // A-packed [T*mtiles][nbf] blocks
    int B, Bpad, T, nbf, precision;
    int seg;         // frames per workgroup (a workgroup walks a time segment of its 16 streams)
    int write_spec;  // 0: the synthesis kernel rebuilds the spectrum from the PCM, nothing is stored
    // optional (one-frame calls, front-end over several frames): `feat` is the LAST slot of a feature history of hist_slots + 1
    // frames [slot][mtiles][nbf]; before it is written the workgroup rolls its m-tile's history by one frame (slots 1 .. hist_slots
    // -> 0 .. hist_slots - 1), so that afterwards the slots are the front-end's taps, oldest first -- no copy launches
    void *feat_hist = nullptr;
    int hist_slots = 0;
    // a SLICE of frames of a longer call (the layer pipeline of mid-size batches, kns_engine.cpp): `pcm` points at the slice's first frame,
    // rows are `pitch` frames apart (0: T), the frame in front of the slice is read from the row itself instead of `hist_in`, and only the
    // call's last slice leaves the history behind
    int pitch = 0, prev_in_pcm = 0, write_hist = 1;
    // optional (calls with per-frame stream resets): the rows that restart at frame t of this launch are the set bits of
    // resets[mtile * rs_pitch + rs_t0 + t] (bit r = stream 16 mtile + r, kns_engine.cpp, ResetRing); in such a frame a row's previous
    // frame is zero.  Selects the kernels' reset arms (a null pointer: the arms are not instantiated in the launch)
    const unsigned *resets = nullptr;
    int rs_pitch = 0, rs_t0 = 0;
};
void launch_analysis(const AnalysisArgs &a, hipStream_t s);

// a stream's comfort-noise setting as the kernels read it (SynthesisArgs::comfort_set, ComfortArgs)
struct ComfortSetting {
    int32_t on;
    uint32_t seed;
};

// ---- synthesis: mask x spectrum -> iFFT -> window -> overlap-add -> int16
struct SynthesisArgs {
    const float *spec;      // as above
    const float *mask;      // C-packed [T*mtiles][17][64][4]: fp32, or fp16 (mask_fp16: the bf16 configuration's mask storage type)
    const float *window;    // [512]
    const float *twiddle;   // [512][2]
    const float *tail_in;   // [Bpad][256] overlap-add state left by the previous call
    float *tail_out;        // [Bpad][256] state after this call (ping-pong with tail_in)
    int16_t *out;           // [B][T*256]
    int B, Bpad, T;
    int seg;                // frames per workgroup; segments after the first replay one frame to rebuild the tail
    const int16_t *pcm;     // recompute != 0: the call's input [B][T*256] ...
    const int16_t *hist_in; // ... and the history the analysis kernel started from, [Bpad][256]
    int recompute;          // rebuild each frame's spectrum from its PCM instead of reading `spec`
    int mask_fp16 = 0;
    // optional (one-frame calls, bf16, stored spectrum): the mask head sigmoid(h . W_mask + b_mask) inside this launch -- four
    // further waves compute the workgroup's mask tile into LDS while the STFT waves fetch their operands; `mask` is not read then
    // a slice of frames of a longer call: `pcm` / `out` point at the slice's first frame, rows `pitch` frames apart (0: T); recompute: the
    // frame in front of the slice comes from the `pcm` row itself instead of `hist_in`
    int pitch = 0, prev_in_pcm = 0;
    const void *mask_h = nullptr;    // A-packed hidden sequence of the last stage's layer B [mtiles][9]
    const void *mask_w = nullptr;    // B-packed [17][9]
    const float *mask_b = nullptr;   // [17 * 16]
    // optional: per-frame stream resets, as in AnalysisArgs -- a resetting row's overlap-add tail and (recompute) previous frame are
    // zero in its reset frame
    const unsigned *resets = nullptr;
    int rs_pitch = 0, rs_t0 = 0;
    // optional: per-stream minimum mask gain, float [Bpad] in [0, 1] (rows past B: 0).  Row b's mask value m becomes g_b + (1 - g_b) m, two
    // roundings, in all 257 bins, before Y = mask . X.  Selects the kernels' kMinGain arm (a null pointer: today's instantiations)
    const float *min_gain = nullptr;
    // optional: the frame report, float [B][T][4] in the caller's layout (e_in, e_out, mask_sum, 0 of every emitted
    // frame).  Points at the slice's first frame like `out`, rows `pitch` frames apart (0: T).  Selects the kernels' kReport arm (a null
    // pointer: today's instantiations)
    float *report = nullptr;
    // optional: linked channels (eighth extension): C = 2, 4 or 8, the rows of a group g C .. g C + C - 1 lie in one mask
    // tile, and every row's mask value becomes the max over its group's, in all 257 bins, behind the report's mask_sum and in front of the
    // minimum gain.  Selects the kernels' kLink arm, which reads `min_gain` (not null then); 0: today's instantiations
    int link = 0;
    // optional: per-stream band profile (tenth extension), float [Bpad][kProfileRow] in the order of profile_index
    // below.  Row b's mask value of bin k becomes min(ceil_b[k], max(floor_b[k], m')) behind the minimum gain and in front of Y = mask . X
    // (and of the report's e_out).  Selects the kernels' kProfile arm, which reads `min_gain` (not null then) and has no linked form
    // (link == 0); a null pointer: today's instantiations
    const float *profile = nullptr;
    // optional: comfort noise (twelfth extension).  comfort_amp: float [Bpad][kComfortRow], every stream's amplitude
    // curve in the order of comfort_index below; comfort_set: [Bpad] (rows past B: off); comfort_n: uint32, the counter value of every
    // frame, pointing at the slice's first frame like `report`, rows `pitch` frames apart (0: T), Bpad rows.  In every frame of a row whose
    // `on` is set Y[k] = m'[k] X[k] + ((1 - m'[k]) A[k]) z[k], z the hash of (seed, n, k) -- behind the profile's clamp, in front of the
    // report's e_out.  Selects the kernels' kComfort arm, which reads `min_gain` and `profile` (neither null then; link == 0); a null
    // comfort_amp: today's instantiations
    const float *comfort_amp = nullptr;
    const ComfortSetting *comfort_set = nullptr;
    const uint32_t *comfort_n = nullptr;
};
void launch_synthesis(const SynthesisArgs &a, hipStream_t s);

// A stream's row of the comfort-noise amplitude table: laid out like the profile's -- the lane of
// column c owns the bins c + 16 k2, four 16-byte words in a row -- and the row ends with one word {A[256], 0, 0, 0}.
constexpr int kComfortRow = 16 * 16 + 4;
inline int comfort_index(int k) { return k == kBins - 1 ? 16 * 16 : (k & 15) * 16 + (k >> 4); }
// ---- comfort noise, the small launch in front of the call (kns_comfort.hip): one lane per stream walks the call's control bytes (the
// leveller's layout) and writes the counter value of every frame, and the counter behind the call
struct ComfortArgs {
    const ComfortSetting *set;  // [Bpad]
    uint32_t *state;            // [Bpad]: n_b -- updated in place (held: untouched; off: no frame counts, a per-frame reset still makes it 0)
    const uint8_t *ctl;         // [B][T + 1] or nullptr (all zero): hold[b], then the call's reset flags of frames 0 .. T - 1
    uint32_t *n;                // [Bpad][T]: the counter value of frame t of stream b (rows past B: 0)
    int B, Bpad, T;
};
void launch_comfort(const ComfortArgs &a, hipStream_t s);
// the counters of the streams with mask[b] != 0 (null: all) := 0
void launch_comfort_reset(uint32_t *state, const uint8_t *mask, int Bpad, hipStream_t s);

// A stream's row of the band-profile table, in the order the synthesis kernel's lanes consume it: the lane of column c owns the bins
// c + 16 k2, k2 = 0 .. 15 -- its 16 floors, then its 16 ceilings, eight 16-byte words in a row -- and the row ends with one word
// {floor[256], ceil[256], 0, 0} that all 16 lanes read.  which: 0 the floor, 1 the ceiling.
constexpr int kProfileRow = 16 * 32 + 4;
inline int profile_index(int k, int which) { return k == kBins - 1 ? 16 * 32 + which : (k & 15) * 32 + which * 16 + (k >> 4); }

// ---- GEMM over all stream-frames: out = act(A . W + bias), A from up to two A-packed sources
enum GemmOut {
    kOutGi = 0,        // C-packed pre-activations (fp32 or fp16), no activation
    kOutMask = 1,      // C-packed, sigmoid: fp32 (fp32 configuration) or fp16 (bf16 configuration: half the bytes of the mask hand-off)
    kOutAPlain = 2,    // A-packed operand type, no activation
    kOutASigmoid = 3,  // A-packed operand type, sigmoid
};
struct GemmArgs {
    const void *a0;   // [mtiles][nb0] blocks (may be null when nb0 == 0)
    const void *a1;   // [mtiles][nb1] blocks
    const void *w;    // B-packed [ntiles][nb0 + nb1] blocks
    const float *bias;  // [ntiles * 16]
    void *out;
    int nb0, nb1;
    int mtiles, ntiles;
    int n_valid;  // logical output width; columns >= n_valid are written as 0 in A-packed outputs
    int out_kind, precision;
    int dev = 0;  // DevVariant bits
    // front-end over several stacked feature frames (KNS-v1.1): the a1 part of A is `taps` blocks of nb1 k-blocks, block i
    // read from a1 + i * tap_stride bytes (the same feature buffer, one frame further on): K = nb0 + taps * nb1 k-blocks
    int taps = 1;
    size_t tap_stride = 0;
    // kOutASigmoid only, optional: instead of whole A-packed blocks of their own, the n_valid (<= kYPadMax) output columns are
    // written INTO block pad_blk of an existing A-packed matrix with pad_nb blocks per m-tile, at columns pad_kk0 ... of that block
    // (2-byte elements; everything else of the block is left alone) -- a narrow head's values in the padding of the feature matrix
    int pad_nb = 0, pad_blk = 0, pad_kk0 = 0;
    // workgroups of the weight-stationary kernels (0: one per CU, 256).  The layer pipeline of mid-size batches launches them narrower,
    // beside the recurrent launches of other layers that hold most of the chip: a grid that does not fit waits for whole CUs
    int grid = 0;
};
void launch_gemm(const GemmArgs &a, hipStream_t s);

// ---- recurrent half of one GRU layer over T frames
struct GruArgs {
    const void *gi;     // C-packed [T][mtiles][51] tiles of (x . W_ih + b_ih)
    const void *whh;    // B-packed [51][nbh] blocks
    const float *bhh;   // [51 * 16]
    const float *hstate_in;  // C-packed fp32 [mtiles][17][64][4]: hidden state before this call
    float *hstate_out;       // the same after this call (ping-pong with hstate_in: the small-batch kernel reads whole
                             // state tiles in every workgroup, so it may not be updated in place)
    void *hseq;         // A-packed [T][mtiles][nbh] blocks, out
    int T, mtiles, precision;
    int dev = 0;  // DevVariant bits
    // optional (bf16 resident kernel): the stage's NARROW head (at most kYPadMax values) computed inside this launch, step by step,
    // from the hidden vectors while they are in LDS -- y_t = sigmoid(h_t . W_head + b_head) written into columns y_kk0 ... of block
    // y_blk of an A-packed matrix with y_nb blocks per m-tile and T x mtiles m-tiles (the feature matrix' padding, kns_layout.h): no
    // head launch, no second pass over the hidden sequence -- and no hidden sequence: with yw set, hseq is neither read nor written
    const void *yw = nullptr;    // B-packed head weights, n-tile 0: [nbh] blocks
    const float *yb = nullptr;   // [16]
    void *yout = nullptr;
    int yvalid = 0, y_nb = 0, y_blk = 0, y_kk0 = 0;
    // optional: per-frame stream resets, as in AnalysisArgs -- before step t, h_{t-1} of the rows that restart at t is zero (bf16:
    // gru_resident8_kernel, fp32: gru_kernel<PF32, 8>; developer A/B switches are not honoured then)
    const unsigned *resets = nullptr;
    int rs_pitch = 0, rs_t0 = 0;
};
void launch_gru(const GruArgs &a, hipStream_t s);

// ---- a whole GRU layer (input GEMM + recurrent step + gates) for ONE frame of a few m-tiles: the low-latency path.
// One wavefront per (unit tile, m-tile): 17 x mtiles workgroups each stream only their 3 n-tiles of W_ih and W_hh.
struct GruSmallArgs {
    const void *a0;     // A-packed y_prev [mtiles][nb0] (null when nb0 == 0)
    const void *a1;     // A-packed e or previous layer's h [mtiles][nbh]
    const void *wih;    // B-packed [51][nb0 + nbh]
    const float *bih;   // [51 * 16]
    const void *whh;    // B-packed [51][nbh]
    const float *bhh;   // [51 * 16]
    const float *hstate_in;
    float *hstate_out;
    void *hseq;         // A-packed [mtiles][nbh], out (this frame's h as the next kernel's A operand)
    int nb0, mtiles, precision;
    // optional: the narrow head of the PREVIOUS stage computed inside this launch (y_prev = sigmoid(h_B . W_head + b_head) of the
    // workgroup's m-tile, every workgroup for itself); a0 is not read then
    const void *yh = nullptr;    // A-packed hidden sequence of the previous stage's layer B [mtiles][nbh]
    const void *yw = nullptr;    // B-packed head weights [n-tiles][nbh]
    const float *yb = nullptr;
    int yvalid = 0;              // head width (columns >= yvalid are zero)
};
void launch_gru_small(const GruSmallArgs &a, hipStream_t s);

// the wavefront form of multi-frame calls (kns_gru.hip, gru_wave_kernel): the items of one anti-diagonal of (pipeline stage, frame)
struct GruWaveItem {
    GruSmallArgs g;     // a GRU layer of one frame: as for launch_gru_small (a0 = the y operand of that frame, read from memory)
    const void *hprev = nullptr;  // A-packed h_{t-1} of this layer [m-tiles][NBH]: the hidden sequence's slot of frame t - 1, or the converted state
    // a narrow head of one frame instead (chains > 0): g.yh / yw / yb / yvalid, g.mtiles; its n-tiles = chains
    int chains = 0;
    int pad = 0;        // 1: the values go into columns y_kk0 ... of block y_blk of `yout` = the features [m-tiles][y_nb] (bf16)
    void *yout = nullptr;  // else: A-packed y operand [m-tiles][y_nb]
    int y_nb = 0, y_blk = 0, y_kk0 = 0;
};
constexpr int kWaveItems = 11;  // eight layers + three heads
struct GruWaveArgs {
    GruWaveItem item[kWaveItems];
    int layer_item[8];  // per XCD: the layer item its workgroups run (-1: none in this launch)
    int head_item[8];   // per XCD: a head item behind the layer's workgroups (-1: none)
    int layer_part[8];  // per XCD: which of the `parts` shares of its layer's workgroups it runs
    int parts;          // XCDs per layer in this launch: 1, 2, 4 or 8
    int layer_wgs;      // workgroups of a layer item = 17 x ceil(mtiles / mgroup)
    int xcd_wgs;        // layer workgroups per XCD = ceil(layer_wgs / parts)
    int mgroup;         // m-tiles per workgroup of a layer item
    int stamp = 0;      // -DKNS_TIMING builds: this launch writes the s_memtime stamps
};
void launch_gru_wave(const GruWaveArgs &w, int precision, int mtiles, hipStream_t s);
// the recurrent state [layers x mtiles][17 tiles] as A-packed operand blocks [layers x mtiles][NBH] (a wavefront call's frame 0)
void launch_gru_wave_prev(const float *hstate, void *hprev, int layers_x_mtiles, int precision, hipStream_t s);

// ---- a whole GRU layer of ONE frame in one launch: input GEMM + recurrent GEMM + gates fused over CU quads (kns_gruq.hip).
// Four workgroups on one XCD own four m-tiles (64 streams); workgroup c pulls the columns of W_ih AND W_hh that belong to
// hidden units 64 c .. 64 c + 63 (and serves unit tile 16 for m-tile c) and computes its quarter of h' for all four m-tiles.
struct GruQuadArgs {
    const void *a0;     // A-packed y_prev [mtiles][nb0] (null when nb0 == 0)
    const void *a1;     // A-packed e or the previous layer's hidden sequence [mtiles][9]
    const void *wih;    // B-packed [51][nb0 + 9]
    const float *bih;   // [51 * 16]
    const void *whh;    // B-packed [51][9] (with the bias rows, kns_layout.h kBiasK0)
    const float *bhh;   // [51 * 16] (unused: the bias rides in whh)
    const float *hstate_in;   // C-packed fp32 [mtiles][17][64][4]
    float *hstate_out;
    void *hseq;         // A-packed [mtiles][9], out
    int nb0, mtiles;
    int quad0 = 0;      // first quad of this launch (set by launch_gru_quad: 64 quads per launch)
    unsigned long long *dbg = nullptr;  // developer build: [8 waves][4][8] s_memtime stamps of workgroup `dbg_block`
    int dbg_block = 0;
    // optional: the narrow head of the PREVIOUS stage computed inside this launch instead of in a launch of its own -- y_prev =
    // sigmoid(h_B . W_head + b_head) of the quad's four m-tiles, straight into the staged x operand; a0 is not read then
    const void *yh = nullptr;    // A-packed hidden sequence of the previous stage's layer B [mtiles][9]
    const void *yw = nullptr;    // B-packed head weights [2 nb0][9]
    const float *yb = nullptr;   // [2 nb0 * 16]
    int yvalid = 0;              // head width (columns >= yvalid are zero)
};
// true when the shape is one the fused kernel takes (bf16, m-tiles in whole quads)
bool gru_quad_supported(int precision, int mtiles, int nb0);
void launch_gru_quad(const GruQuadArgs &a, hipStream_t s);

// ---- state reset of selected streams
struct ResetArgs {
    int16_t *hist;   // [Bpad][256] (both ping-pong copies are cleared)
    int16_t *hist2;
    float *tail;     // [Bpad][256] (both ping-pong copies are cleared)
    float *tail2;
    float *hstate;   // [8][mtiles][17][64][4] (both ping-pong copies are cleared)
    float *hstate2;
    const uint8_t *mask;  // [Bpad] device copy, or null for all
    int Bpad;
    // front-end context (KNS-v1.1, front_taps > 1): the features of the last front_taps - 1 frames, A-packed
    // [frames][mtiles][nbf] blocks; a reset stream's rows are set to the feature of a silent frame (`silent`: one A-packed
    // m-tile [nbf] blocks whose 16 rows are all that feature)
    void *fhist = nullptr;
    const void *silent = nullptr;
    int fhist_frames = 0, nbf = 0;
};
void launch_reset(const ResetArgs &a, hipStream_t s);
// ---- per-stream state <-> stream records (kns_state.hip).  A record is self-contained and position-independent (little-endian):
//   header, 32 bytes: magic "KNSS", uint32 version (1), uint32 front_taps, uint32 precision, uint64 model content hash (the hash the
//                     shared weight image is keyed on), 8 reserved zero bytes
//   hist   int16[256]                    the previous frame's samples (the analysis kernel's hist_in)
//   tail   float[256]                    overlap-add tail
//   h      float[8][271]                 hidden state, layer-major, logical unit order (the order of debug tap 3)
//   fctx   float[front_taps - 1][257]    feature context, oldest first (absent for front_taps == 1); bf16 features widened to float
// 10 240 bytes for front_taps == 1.  It does not depend on the batch size, the slot, the m-tile, the ping-pong parity or the route;
// padding rows and columns of the packed layouts never enter it and are left alone on import.  A record belongs to one model and one
// precision: importing into a handle of the other precision is refused (a bf16 handle's feature context is not an fp32 handle's).
constexpr uint32_t kStateMagic = 0x53534e4bu;  // "KNSS"
constexpr uint32_t kStateVersion = 1;
// Version 2, of handles that are not at 16 kHz: the first four reserved header bytes hold uint32 sample_rate, and behind the version-1 parts
// follow rs_in and rs_out, int16, oldest first (the sample-rate stages' histories, below), zero-padded to whole 16-byte words: 288 bytes at
// 8 and 32 kHz, 384 at 48 kHz, 224 at 12 kHz, 240 at 24 kHz.  A 16 kHz handle writes and accepts version 1 only, a handle at another rate version 2 of its own rate.
constexpr uint32_t kStateVersionRate = 2;
constexpr int kStateHeaderBytes = 32, kStateHistOff = 32, kStateTailOff = kStateHistOff + kFrame * 2,
              kStateHOff = kStateTailOff + kFrame * 4, kStateFctxOff = kStateHOff + kGruLayers * kHidden * 4;
static_assert(kStateFctxOff == 10240 && kStateFctxOff % 16 == 0 && (kBins * 4 * 4) % 16 == 0, "stream record layout");
KNS_HD size_t state_record_bytes(int front_taps) {  // whole 16-byte words (front_taps 2 ... 4: up to 12 trailing zero bytes)
    return ((size_t) kStateFctxOff + (size_t) (front_taps - 1) * kBins * 4 + 15) / 16 * 16;
}
struct StateArgs {
    int16_t *hist[2];   // [Bpad][256]; [0] = the current ping-pong copy (export reads it; import writes both)
    float *tail[2];     // [Bpad][256]
    float *hstate[2];   // C-packed [8][mtiles][17][64][4]
    void *fhist;        // A-packed [front_taps][mtiles][nbf] blocks (slot 0 is the one-frame roll's spare: not part of the state)
    const int32_t *rec_of;  // [Bpad]: the record of stream b in `records`, -1 = not listed (the inverse of the caller's stream list)
    uint8_t *records;   // [count][state_bytes], device memory
    uint4 hdr0, hdr1;   // the 32 header bytes (export)
    uint32_t state_bytes;
    int Bpad, nbf, precision, taps;
};
void launch_state_export(const StateArgs &a, hipStream_t s);
void launch_state_import(const StateArgs &a, hipStream_t s);
// ---- sample-rate stages of handles that are not at 16 kHz (kns_resample.hip; DESIGN.md section 2, third extension).  A handle runs two
// stages "up U, down D": the in-stage from its rate to 16 kHz and the out-stage, the same pair swapped, back.  (R, 1) is the interpolator,
// (1, R) the decimator (8, 32 and 48 kHz: R = 2, 2, 3); 12 and 24 kHz go through the common rate 48 kHz with (4, 3) and (2, 3).  A stage's
// prototype has L = 48 K + 1 taps, K = max(U, D), and the stage keeps its last (L - 1) / U input samples per stream, int16, oldest first.
// At 12 / 24 kHz: 48 in, 64 out / 72 in, 48 out; frame_length 192 / 384, delay_sample 192 + 24 + 24 = 240 / 384 + 36 + 36 = 456,
// version-2 record tail 224 / 240 bytes, state_size 10 464 / 10 480 for a one-frame front-end.
constexpr int kRate16k = 16000, kRsHalf = 24, kRsMaxTaps = 2 * kRsHalf * 4 + 1;
struct RsStage {
    int U, D;  // up U, down D
};
KNS_HD constexpr RsStage rs_stage_in(int rate) {
    return rate == 8000 ? RsStage{2, 1} : rate == 32000 ? RsStage{1, 2} : rate == 48000 ? RsStage{1, 3} : rate == 12000 ? RsStage{4, 3} :
           rate == 24000 ? RsStage{2, 3} : rate == kRate16k ? RsStage{1, 1} : RsStage{0, 0};
}
KNS_HD constexpr RsStage rs_stage_out(int rate) { return RsStage{rs_stage_in(rate).D, rs_stage_in(rate).U}; }
KNS_HD constexpr bool rs_rate_ok(int rate) { return rs_stage_in(rate).U != 0; }
KNS_HD constexpr int rs_frame_length(int rate) { return rate / 1000 * kFrame / 16; }  // 128 / 192 / 256 / 384 / 512 / 768
KNS_HD constexpr int rs_stage_hist(RsStage s) { return 2 * kRsHalf * (s.U > s.D ? s.U : s.D) / s.U; }  // (L - 1) / U
KNS_HD constexpr int rs_in_hist(int rate) { return rate == kRate16k ? 0 : rs_stage_hist(rs_stage_in(rate)); }
KNS_HD constexpr int rs_out_hist(int rate) { return rate == kRate16k ? 0 : rs_stage_hist(rs_stage_out(rate)); }
// what both stages add to a stream's delay, in samples at the handle's rate: each stage 24 K samples at the stages' common high rate,
// U_in times the handle's -- together 48 K / U_in, which is the in-stage's history
KNS_HD constexpr int rs_delay(int rate) { return rs_in_hist(rate); }
// the part of a version-2 stream record behind the version-1 parts: rs_in, rs_out, zero-padded to whole 16-byte words
KNS_HD constexpr size_t rs_record_bytes(int rate) { return ((size_t) (rs_in_hist(rate) + rs_out_hist(rate)) * 2 + 15) / 16 * 16; }
KNS_HD size_t state_record_bytes(int front_taps, int rate) { return state_record_bytes(front_taps) + rs_record_bytes(rate); }
static_assert(rs_in_hist(8000) == 48 && rs_out_hist(8000) == 96 && rs_in_hist(32000) == 96 && rs_out_hist(32000) == 48 &&
              rs_in_hist(48000) == 144 && rs_out_hist(48000) == 48 && rs_in_hist(12000) == 48 && rs_out_hist(12000) == 64 &&
              rs_in_hist(24000) == 72 && rs_out_hist(24000) == 48 && rs_in_hist(kRate16k) == 0 && rs_out_hist(kRate16k) == 0, "stage histories");
static_assert(rs_delay(8000) == 48 && rs_delay(32000) == 96 && rs_delay(48000) == 144 && rs_delay(12000) == 48 && rs_delay(24000) == 72 &&
              rs_delay(kRate16k) == 0 && rs_record_bytes(8000) == 288 && rs_record_bytes(32000) == 288 && rs_record_bytes(48000) == 384 &&
              rs_record_bytes(12000) == 224 && rs_record_bytes(24000) == 240, "stage constants");
// a stage "up U, down D": out[n] = sum over i = D n mod U, + U, ... < L of taps[i] a[(D n - i) / U].  A frame is q_frame groups of D input
// and U output samples.
struct ResampleArgs {
    const int16_t *in;      // [B][T * D q_frame] (caller layout)
    int16_t *out;           // [B][T * U q_frame]
    const int16_t *state;   // [Bpad][(L - 1) / U]: the stream's last input samples before the call, oldest first
    int16_t *state_next;    // the same after the call: the other copy of the ping-pong pair
    const uint8_t *resets;  // optional, device memory [B][T]: non-zero at [b][t] = everything in front of block t of stream b reads as zero
    int B, T, U, D, q_frame;
    float taps[kRsMaxTaps];  // h_U[i] = (float) (U g[i]), L = 48 max(U, D) + 1 of them, zero-padded: wave-uniform, read from the argument segment
};
void launch_resample(const ResampleArgs &a, hipStream_t s);
// state rows [Bpad][hist], both copies, of the streams with mask[b] != 0 (null: all) := 0
void launch_resample_reset(int16_t *state0, int16_t *state1, int hist, const uint8_t *mask, int Bpad, hipStream_t s);
// the rs part of stream records [count][rec_bytes] (device) <- / -> the two state arrays, for the streams with rec_of[b] >= 0
struct ResampleStateArgs {
    int16_t *state_in[2], *state_out[2];  // [Bpad][hist_in], [Bpad][hist_out]; [0] = the current copy (export reads it; import writes both)
    int hist_in, hist_out;
    const int32_t *rec_of;          // [Bpad]
    uint8_t *records;
    uint32_t rec_bytes;
    int Bpad, import;               // import != 0: records -> state
};
void launch_resample_state(const ResampleStateArgs &a, hipStream_t s);
// ---- packet handles (kns_packet.hip; DESIGN.md section 2, fourth extension): streams that take and deliver any number of samples per call.
// Per stream on top of everything above: fill = (samples since the last reset) mod F, `fill` pending input samples and F - 1 - fill pending
// output samples, oldest first.  On the device the two parts are two rows of F int16 (pin, pout: each kernel rewrites its own in place) with
// a length each (fill_in, fill_out: equal between calls, apart only between a call's two kernels).
// Version 3, of packet handles: the header's sample_rate field is always set, and behind the version-1 (16 kHz) or version-2 parts follow
// uint32 fill and int16[F - 1] = [pending input | pending output], zero-padded to whole 16-byte words: 272 / 528 / 1040 / 1552 bytes.
constexpr uint32_t kStateVersionPacket = 3;
KNS_HD size_t pk_record_bytes(int rate) { return ((size_t) 4 + (size_t) (rs_frame_length(rate) - 1) * 2 + 15) / 16 * 16; }
struct PacketArgs {
    const int16_t *user_in;  // [B][max_samples]: row b's first tab[b] samples count (packet_in_kernel)
    int16_t *user_out;       // [B][max_samples]: row b's first tab[b] samples are written (packet_out_kernel)
    // the call's table, device memory: int32 counts[Bpad], nsub, cut[nsub + 1] (sub-call l = frames [cut[l], cut[l + 1]) of the call)
    const int32_t *tab;
    int16_t *pin, *pout;          // [Bpad][F]
    int32_t *fill_in, *fill_out;  // [Bpad]
    // the sub-calls' dense frame matrices [B][T_l F], stacked: sub-call l starts B F cut[l] samples in (in: their input, out: their output)
    int16_t *frames;
    const float *sub_report;  // the sub-calls' reports [B][T_l][4], stacked the same way
    float *report;            // optional: [B][report_frames][4], stream b's rows [0, k_b) are written
    int report_frames, max_samples, B, Bpad, F;
};
void launch_packet_in(const PacketArgs &a, hipStream_t s);
void launch_packet_out(const PacketArgs &a, hipStream_t s);
struct PacketStateArgs {
    int16_t *pin, *pout;
    int32_t *fill_in, *fill_out;
    const int32_t *rec_of;  // [Bpad] (launch_packet_state)
    uint8_t *records;       // the packet part of stream records [count][rec_bytes] (device)
    uint32_t rec_bytes;
    int Bpad, F, import;
};
void launch_packet_reset(const PacketStateArgs &a, const uint8_t *mask, hipStream_t s);  // mask: device [Bpad], null: every stream
void launch_packet_state(const PacketStateArgs &a, hipStream_t s);
// ---- fractional sample-rate stages of packet handles at 44 100 and 22 050 Hz (kns_fractional.hip; DESIGN.md section 2, sixth extension).
// 16 000 / 44 100 = 160 / 441 and 16 000 / 22 050 = 320 / 441: the in-stage is "up U, down 441", the out-stage "up 441, down U", over the
// prototype of K = 441 (L = 21 169 taps), around the unchanged 16 kHz packet path.  Consecutive outputs sit at different phases, so the
// taps are per-lane loads from a polyphase table in global memory, [tap j][phase r] = h[r + P j] (P = U in, 441 out; zero where r + P j >= L).
// Per stream: N mod 441 (one copy per stage: they differ between a call's two launches), the in-stage's last fr_in_taps(U) input samples
// and the out-stage's last kFrOutHist inner output samples, int16, oldest first.
constexpr int kFrDown = 441, kFrTaps = 2 * kRsHalf * kFrDown + 1, kFrInnerDelay = 2 * kFrame - 1, kFrOutTaps = 49, kFrOutHist = 49;
constexpr int kFrMaxSamples = 1 << 22;  // the most samples per call of such a handle: U (441 + n) stays an int
KNS_HD constexpr int fr_up(int rate) { return rate == 44100 ? 160 : rate == 22050 ? 320 : 0; }
KNS_HD constexpr bool fr_rate_ok(int rate) { return fr_up(rate) != 0; }
KNS_HD constexpr int fr_in_taps(int U) { return (kFrTaps + U - 1) / U; }  // 133 / 67: the most taps of an in-stage output, and its history
// the chain's delay in ticks of 1 / (U rate): both stages' 24 * 441 and the inner packet handle's 511 * 441
KNS_HD constexpr int fr_ticks() { return (2 * kRsHalf + kFrInnerDelay) * kFrDown; }
KNS_HD constexpr int fr_shift(int U) { return (U - fr_ticks() % U) % U; }  // c: the out-stage's time base, U n - c
KNS_HD constexpr int fr_delay(int U) { return (fr_ticks() + fr_shift(U)) / U; }
// M(N) = ceil(U N / 441): the inner samples that exist once a stream has received N samples
KNS_HD constexpr long long fr_inner(long long n, int U) { return (U * n + kFrDown - 1) / kFrDown; }
static_assert(fr_in_taps(160) == 133 && fr_in_taps(320) == 67 && fr_shift(160) == 41 && fr_shift(320) == 201 && fr_delay(160) == 1541 &&
              fr_delay(320) == 771 && kFrTaps == 21169 && (kFrTaps + kFrDown - 1) / kFrDown == kFrOutTaps, "fractional stage constants");
struct FractionalArgs {
    const int16_t *in;      // in-stage: [B][in_stride] at the handle's rate, row b's first counts[b] samples; out-stage: the inner output,
                            // row b's first M(phase + counts[b]) - M(phase) samples
    int16_t *out;           // [B][out_stride]: the other of the two
    const int32_t *counts;  // device [Bpad]: the call's samples per stream at the handle's rate
    int16_t *hist;          // [Bpad][fr_in_taps(U)] or [Bpad][kFrOutHist], rewritten in place (one workgroup owns a stream)
    int32_t *phase;         // [Bpad]: N mod 441, this stage's copy
    const float *taps;      // [fr_in_taps(U)][U] or [kFrOutTaps][441]
    int in_stride, out_stride, U;
};
void launch_fractional_in(const FractionalArgs &a, int B, hipStream_t s);
void launch_fractional_out(const FractionalArgs &a, int B, hipStream_t s);
struct FractionalStateArgs {
    int16_t *hist_in, *hist_out;
    int32_t *phase_in, *phase_out;
    int taps_in, Bpad;
};
void launch_fractional_reset(const FractionalStateArgs &a, const uint8_t *mask, hipStream_t s);  // mask: device [Bpad], null: every stream
// ---- sample formats of batch handles (kns_format.hip; DESIGN.md section 2, fifth extension): what a caller's `pcm` and `enhanced` hold.
// Configuration of the handle, not stream state: the engine's samples are int16 whatever the format, which is a conversion on the device in
// front of and behind the unchanged call.  The values are pv_koala_sample_format_t's.
enum SampleFormat { kFmtS16 = 0, kFmtF32 = 1, kFmtUlaw = 2, kFmtAlaw = 3 };
KNS_HD bool fmt_ok(int fmt) { return fmt >= kFmtS16 && fmt <= kFmtAlaw; }
KNS_HD int fmt_bytes(int fmt) { return fmt == kFmtS16 ? 2 : fmt == kFmtF32 ? 4 : 1; }  // bytes per element
KNS_HD int fmt_group(int fmt) { return fmt == kFmtF32 ? 8 : 16; }                       // elements one lane converts
struct FormatArgs {
    const void *in;         // [rows][n] dense: the format's elements (format_in) or int16 (format_out), aligned to the element only
    void *out;              // [rows][n] dense: int16 (format_in) or the format's elements (format_out), aligned to the element only
    const int32_t *counts;  // device [rows] or nullptr: row b's first counts[b] elements are converted and written (nullptr: all n)
    long long n;
    int rows;
};
// fmt: kFmtF32, kFmtUlaw or kFmtAlaw (an S16 handle launches neither)
void launch_format_in(int fmt, const FormatArgs &a, hipStream_t s);
void launch_format_out(int fmt, const FormatArgs &a, hipStream_t s);
// ---- multi-channel batch handles (kns_channels.hip; DESIGN.md section 2, seventh extension): the caller's `pcm` and `enhanced` hold the C
// streams of a group interleaved.  Configuration of the handle, not stream state: the layout of two buffers and nothing else -- a split in
// front of and a join behind the unchanged call, on elements of `width` = 1, 2 or 4 bytes (the handle's format).
constexpr int kChannelsMax = 8;
constexpr int kChSpanBytes = 8192;  // a workgroup's span of one group, all channels
KNS_HD int ch_span(int C, int width) { return (kChSpanBytes / (C * width)) & ~15; }  // ... in samples per channel: whole 16-byte words of a row
struct ChannelArgs {
    const void *in;         // split: [G][n C] interleaved; join: [G C][n] rows -- dense, aligned to the element only
    void *out;              // split: [G C][n] rows; join: [G][n C] interleaved
    const int32_t *counts;  // join: device [G C] or nullptr: group g's first counts[g C] C elements are written (nullptr: all n C)
    long long n;            // samples per stream
    int G, C;               // groups, channels (2 .. kChannelsMax)
};
void launch_channels_split(int width, const ChannelArgs &a, hipStream_t s);
void launch_channels_join(int width, const ChannelArgs &a, hipStream_t s);
// ---- high-band carry (kns_highband.hip; DESIGN.md section 2, ninth extension): frame handles at 32 and 48 kHz add the band the 16 kHz
// call never saw, delayed like the call and scaled by a broadband gain from the call's own masks, to the out-stage's result -- one launch
// behind the out-stage.  R = rate / 16000.  Per stream, held only while the feature is on: the last hb_x_hist(R) input samples, the last
// kHbYHist in-stage outputs (one engine frame and the out-stage's history) and the broadband gains s' of the last two frames.
constexpr int kHbYHist = kFrame + 2 * kRsHalf;  // 304
KNS_HD constexpr bool hb_rate_ok(int rate) { return rate == 32000 || rate == 48000; }
KNS_HD constexpr int hb_x_hist(int R) { return kHbYHist * R; }  // = delay_sample: 608 / 912
struct HighBandArgs {
    const int16_t *x;       // [B][T 256 R]: the call's input at the handle's rate
    const int16_t *y;       // [B][T 256]: the in-stage's output of the call
    int16_t *out;           // [B][T 256 R]: the out-stage's result E, rewritten in place
    const float *report;    // [B][T][4]: the call's frame report (row [b][t][2] = mask_sum)
    const float *min_gain;  // [Bpad] or nullptr (every gain 0): the call's attenuation limit
    const uint8_t *resets;  // [B][T] or nullptr: a stream with resets[b T] != 0 is fresh in front of the call (later frames: refused above)
    const int16_t *xs, *ys;  // the state in front of the call: [Bpad][hb_x_hist(R)], [Bpad][kHbYHist], oldest first
    const float *ss;         // [Bpad][2]: s' of the frame before the call, and of the one before that
    int16_t *xs_next, *ys_next;  // ... behind it (the other copy of the ping-pong pair)
    float *ss_next;
    int B, T, R;
    int link;  // channels of a linked group (the gain's s is the max over the group's), 0 or 1: none
    float taps[kRsMaxTaps];  // the out-stage's table h_R, as ResampleArgs'
};
void launch_high_band(const HighBandArgs &a, hipStream_t s);
// both copies of the three state arrays of the streams with mask[b] != 0 (null: all) := 0
void launch_high_band_reset(int16_t *const xs[2], int16_t *const ys[2], float *const ss[2], int R, const uint8_t *mask, int Bpad, hipStream_t s);
// ---- output leveller (kns_level.hip; DESIGN.md section 2, eleventh extension): a per-stream, speech-gated automatic gain on the samples of
// the 16 kHz call, from the call's own frame report -- two launches directly behind the call.  Per stream: a setting (configuration, the
// owner's, like the attenuation limit) and two floats of state, lvl (the tracked speech energy) and gain; fresh: (0, 1).
struct LevelSetting {
    int32_t on;
    float target, max_boost, max_cut, theta, e_floor, a_up, a_down, slew;
};
struct LevelArgs {
    const LevelSetting *set;  // [Bpad]
    float *state;             // [Bpad][2]: lvl, gain -- updated in place (streams that are off or held: untouched)
    const uint8_t *ctl;       // [B][T + 1] or nullptr (all zero): hold[b], then the call's reset flags of frames 0 .. T - 1
    const float *report;      // [B][T][4]: the call's frame report (e_out, mask_sum)
    float *report_out;        // the caller's report (then == report) or nullptr: column 3 of a levelling stream's rows := g_t
    float *gains;             // scratch [B][T][2]: the gains at the first and behind the last sample of every frame
    int16_t *out;             // [B][T 256]: the call's samples E, rewritten in place
    int B, T;
};
void launch_level(const LevelArgs &a, hipStream_t s);  // the tracker, then the ramp over the samples
// the state of the streams with mask[b] != 0 (null: all) := fresh
void launch_level_reset(float *state, const uint8_t *mask, int Bpad, hipStream_t s);
// ---- peak limiter (kns_limit.hip; DESIGN.md section 2, thirteenth extension): a per-stream ceiling on the samples of the 16 kHz call with
// instant attack and linear release, in the leveller's place -- ONE launch applies the leveller's ramp and the limiter, instead of
// level_apply_kernel.  Per stream: a setting (configuration, the owner's) and one float of state, the gain g behind the last sample; fresh: 1.
struct LimiterSetting {
    int32_t on;
    float ceiling, release;  // c in sample units, 1 <= c <= 32767; the gain recovered per sample, 0 < release <= 1
};
struct LimitArgs {
    const LimiterSetting *set;  // [Bpad]
    float *state;               // [Bpad]: g -- updated in place (streams that are off or held: untouched)
    const uint8_t *ctl;         // [B][T + 1] or nullptr (all zero): the leveller's control rows
    const float *gains;         // [B][T][2], the tracker's pairs of this call, or nullptr: no stream levels, every pair is (1, 1)
    int16_t *out;               // [B][T 256]: the call's samples E, rewritten in place
    int B, T;
};
void launch_level_track(const LevelArgs &a, hipStream_t s);  // the leveller's tracker alone: the pairs for launch_limit
void launch_limit(const LimitArgs &a, hipStream_t s);        // the leveller's ramp and the limiter over the samples
// g of the streams with mask[b] != 0 (null: all) := 1
void launch_limit_reset(float *state, const uint8_t *mask, int Bpad, hipStream_t s);
// last node of a captured one-frame replay: ++*counter (device memory), published to *host_word (page-locked host memory)
void launch_frame_done(unsigned *counter, unsigned *host_word, hipStream_t s);

}  // namespace kns
