// kns_engine.h -- host-side engine behind both the single-stream and the batch C ABI.
// One Engine = B lock-stepped streams on one GPU: parameter upload (pre-packed for MFMA), per-stream state in HBM,
// activation workspace in fragment layouts, and the per-chunk kernel sequence.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "kns_kernels.h"

namespace kns {

// host copy of a KNS1 parameter file (fp32, logical layout; see koala_amd/params.py)
struct Params {
    // Not part of the file: the sample rate of the handle to be made (8 000, 16 000, 32 000 or 48 000 Hz; DESIGN.md section 2, third
    // extension).  load_params leaves 16 000; the batch C ABI sets it.  It is no part of the content hash: all rates share one weight image.
    int sample_rate = 16000;
    int front_taps = 1;  // feature frames the front-end sees (KNS-v1: 1; KNS-v1.1: up to 5, w_in then has front_taps * 257 rows, oldest frame first)
    int head[kStages];
    std::vector<float> mean, scale, w_in, b_in;
    struct Stage {
        int d_in, d_out;
        std::vector<float> w_ih_a, b_ih_a, w_hh_a, b_hh_a, w_ih_b, b_ih_b, w_hh_b, b_hh_b, w_head, b_head;
    } st[kStages];
};

enum LoadResult { kLoadOk = 0, kLoadIo = 1, kLoadFormat = 2 };
LoadResult load_params(const char *path, Params *out, std::string *err);

constexpr int kNumKernelClasses = 5;
enum KernelClass { kClsAnalysis = 0, kClsGemmIn = 1, kClsGru = 2, kClsGemmHead = 3, kClsSynthesis = 4 };

// The per-stream settings a call carries ("Per-stream settings"): the owner's -- the C ABI's handle, which checks every
// value and counts its changes -- and the same for a frame call and a packet call, whose sub-calls and inner calls take them on as they are.
struct StreamOptions {
    // Per-stream attenuation limit: host memory, float [num_streams], every value in [0, 1] (checked by the owner, the C ABI's handle).
    // Stream b's mask value m becomes min_gain[b] + (1 - min_gain[b]) m in every frame of the call.  Read before
    // the call returns (copied into an upload slot of the call when `min_gain_rev` differs from the one the engine's device table holds: the
    // owner counts its changes).  nullptr: every gain is 0, the plain call -- same route, same kernels, same bits.
    const float *min_gain = nullptr;
    unsigned min_gain_rev = 0;
    // Linked channels (eighth extension; a handle with channels() == 2, 4 or 8 only): non-zero, and the mask applied to
    // a stream in every frame of the call is the max over the masks of its group's streams, bin by bin.  The call then carries `min_gain`
    // (all zero where no limit is in force: the linked kernels read the table), and `hold` must be equal within a group.  The owner's
    // setting, like the limit: the engine keeps nothing of it between calls.  0: the plain call -- same route, same kernels, same bits.
    int channel_link = 0;
    // Band profile (tenth extension): host memory, float [num_streams][kProfileRow] -- every stream's 257 floors and
    // ceilings in the order of profile_index (kns_kernels.h), every value in [0, 1] and floor <= ceiling (checked by the owner, the C ABI's
    // handle).  Stream b's mask value of bin k becomes min(ceil_b[k], max(floor_b[k], m')) in every frame of the call, m' the value under
    // `min_gain`, which the call then carries (all zero where no limit is in force: the profile kernels read that table).  Read before the
    // call returns, like the gains: copied into an upload slot of the call when `band_profile_rev` differs from the one the engine's device
    // table holds.  Not combined with `channel_link` nor with `high_band`.  nullptr: the neutral profile, the plain call -- same route, same
    // kernels, same bits.
    const float *band_profile = nullptr;
    unsigned band_profile_rev = 0;
    // Output leveller (eleventh extension): host memory, LevelSetting [num_streams], every field checked by the owner,
    // the C ABI's handle, which passes the table only while some stream's `on` is set.  Two launches directly behind the 16 kHz call
    // (kns_level.hip) track each levelling stream's speech energy from the call's own frame report and rewrite its samples under a gain
    // ramped over every frame; the state, two floats per stream, is the engine's (level_state, reset, `resets`, `hold`).  Read before the
    // call returns, like the gains: uploaded when `level_rev` differs from the one the engine's device table holds.  Below the host
    // boundary such a call runs on device pointers only.  Not combined with `channel_link`, `high_band` nor process_host_async.
    // nullptr: the plain call -- same launches, same bits, and the state does not move.
    const LevelSetting *level = nullptr;
    unsigned level_rev = 0;
    // Peak limiter (thirteenth extension): host memory, LimiterSetting [num_streams], every field checked by the owner,
    // which passes the table only while some stream's `on` is set.  One launch (kns_limit.hip) directly behind the 16 kHz call, in the
    // place of the leveller's second one, applies the leveller's ramp and holds every limiting stream's samples under its ceiling; the
    // state, one float per stream, is the engine's (limiter_state, reset, `resets`, `hold`).  Uploaded when `limiter_rev` differs from the
    // one the engine's device table holds.  Everything else as `level`: device pointers below the host boundary, not combined with
    // `channel_link`, `high_band` nor process_host_async.  nullptr: the call without it -- same launches, same bits, the state does not move.
    const LimiterSetting *limiter = nullptr;
    unsigned limiter_rev = 0;
    // Comfort noise (twelfth extension): host memory, ComfortSetting [num_streams] and the amplitude curves float
    // [num_streams][kComfortRow] in the order of comfort_index (kns_kernels.h), every value finite and >= 0, checked by the owner, which passes
    // the tables only while some stream's `on` is set -- and then `band_profile` and `min_gain` too (neutral, all zero where none is in force:
    // the comfort kernels carry both).  A small launch in front of the call (kns_comfort.hip) counts every filling stream's frames; the
    // synthesis kernels add the shaped noise where the mask removed energy.  The counter, one uint32 per stream, is the engine's
    // (comfort_state, reset, `resets`, `hold`).  Uploaded when `comfort_rev` differs from the one the engine's device tables hold.  Below the
    // host boundary such a call runs on device pointers only.  Not combined with `channel_link`, `high_band` nor process_host_async.
    // nullptr: the plain call -- same launches, same bits, and the counters do not move.
    const ComfortSetting *comfort = nullptr;
    const float *comfort_amp = nullptr;
    unsigned comfort_rev = 0;
};

// One call that advances the streams, with everything it carries.  pcm/out: [B][T*frame_length] at the handle's sample rate (256 at
// 16 kHz), host or device pointers (both of the same kind).  On a handle with a sample format (Engine::set_format) they point to elements
// of that format -- float or uint8 -- behind the int16 type: the entry casts, and every size is a count of sample_bytes().  Host pointers
// are the entry's business (Engine::process): below it a call of a handle that is not the plain one carries device pointers only.
struct Call {
    int T;
    const int16_t *pcm;
    int16_t *out;
    // Per-frame stream resets: host memory, uint8 [num_streams][T] (non-zero at [b][t]: stream b restarts from the fresh state right before
    // frame t).  Consumed before the call returns -- packed into an upload slot (kns_engine.cpp, begin_resets) -- so the caller may
    // overwrite it then.  nullptr or all zero: the plain call.
    const uint8_t *resets = nullptr;
    // Held streams: host memory, uint8 [num_streams].  The streams with hold[b] != 0 are not advanced: their state after the call is bit for
    // bit what it was before it (exported to a device scratch in front of the whole call and imported back behind it); their rows of `out`
    // are unspecified.  nullptr or all zero: the plain call.  Not combined with `resets`, not taken by process_host_async.
    const uint8_t *hold = nullptr;
    bool host_contract = false;  // pcm/out are host memory by the entry point's contract: no driver query per frame on the latency path
    // Frame report: float [num_streams][T][4], memory of the same kind as `out` (host with host, device with device; process_host_async:
    // page-locked).  Row [b][t] = e_in, e_out, mask_sum, 0 of stream b's frame t (three sums the synthesis kernel
    // forms in a fixed order); complete when `out` is.  An output only: the streams' evolution and `out` do not depend on whether it was asked
    // for.  Held streams' rows are unspecified.  nullptr: the plain call -- same route, same kernels, same bits.
    float *report = nullptr;
    // High-band carry (ninth extension; a frame handle at 32 or 48 kHz only): non-zero, and the band above the stages'
    // pass band is added to `out`, delayed like the call and scaled by a broadband gain from the call's masks (kns_highband.hip).  The
    // owner's setting, like the link; `high_band_epoch` counts the times the owner turned it on: the engine allocates the feature's
    // per-stream state at the first such call and clears it when the epoch is not the one it saw last.  Not combined with `hold`, nor with
    // `resets` behind frame 0.  0: the plain call -- same launches, same bits.
    int high_band = 0;
    unsigned high_band_epoch = 0;
    StreamOptions opt;  // the per-stream settings, above
};

// kBadArgument: a stream list, a record or a combination of Call members that the engine refused before it touched anything (the C ABI
// reports INVALID_ARGUMENT).  kRuntime: a HIP failure, and the refusals the ABI has always reported as a runtime error (pointer kinds,
// overlapping buffers).
enum class Status { kOk, kBadArgument, kRuntime };

// One call of a packet handle (include/pv_koala_batch.h, pv_koala_batch_process_packets): stream b gives and takes counts[b] samples.
// Host pointers end at the entry (Engine::run_packets), which refuses a bad member before anything is enqueued.
struct PacketCall {
    int max_samples;                   // row length of pcm / out, 1 .. the handle's
    const int32_t *counts;             // host [num_streams], each in [0, max_samples]
    const int16_t *pcm;                // [num_streams][max_samples], host or device (elements of the handle's format, as Call's)
    int16_t *out;                      // the same kind
    const uint8_t *restart = nullptr;  // host [num_streams] or nullptr: the stream is fresh before this packet
    float *report = nullptr;           // [num_streams][report_frames][4], memory of out's kind, or nullptr
    int report_frames = 0;
    int32_t *frames = nullptr;         // host [num_streams] or nullptr, out: frames completed by the call
    // as Call's.  `channel_link`: `restart`, and the streams' phase (the mirrors of fill and of N mod 441), must be equal within a group;
    // `level`, `limiter`, `comfort`: not on a handle at 44 100 or 22 050 Hz
    StreamOptions opt;
};

class Engine {
public:
    // returns nullptr and fills *err on failure (*oom set when the failure was an allocation)
    static Engine *create(const Params &p, int device, int num_streams, int max_frames, int precision,
                          std::string *err, bool *oom);
    ~Engine();

    int num_streams() const { return B_; }
    int max_frames() const { return Tmax_; }
    int device() const { return device_; }
    int front_taps() const { return taps_; }
    int sample_rate() const { return rate_; }

    // The two entries that advance the streams.  Host pointers: synchronous.  Device pointers: enqueued.
    Status process(const Call &c, std::string *err);
    // Page-locked host buffers, asynchronous: the call's copy-in, kernels and copy-out are enqueued on three streams and the function
    // returns; up to three such calls are in flight (a fourth first waits for the oldest), so the copies of one call run under the
    // kernels of its neighbours.  `drain_async` (also reached through synchronize(), and entered by every other entry point) waits
    // for all of them.
    Status process_host_async(const Call &c, std::string *err);
    bool drain_async(std::string *err);
    bool async_wait(int max_in_flight, std::string *err);  // until at most that many asynchronous calls are still in flight (0: all done)
    bool reset(const uint8_t *host_mask, std::string *err);
    // 0: back to the handle's own stream.  Waits for everything the handle has in flight first (asynchronous host calls and the work
    // queued on the previous stream, which must still exist: the next call's kernels touch the same state, history and tail buffers)
    void set_stream(hipStream_t s);
    bool synchronize(std::string *err);

    // ---- per-stream state as stream records (kns_kernels.h, StateArgs: the record; kns_state.hip: the kernels).  `records` is HOST memory
    // (pageable or page-locked), count x state_bytes(), record i = stream streams[i] (streams == nullptr: slots 0 .. count - 1).  Both
    // calls first wait for asynchronous host calls in flight, then run on the handle's current stream, through a device staging buffer of
    // num_streams records allocated on first use.  export_state returns when the records are filled.
    // import_state checks every header (magic, version, front_taps, precision, model hash -- a record of the other precision is refused:
    // its feature context is the other engine's) and every index (outside [0, num_streams), the same slot twice) BEFORE anything is written,
    // returns when the host records may be reused, and its scatter is ordered on the stream in front of the next call.  A failed call
    // leaves all state as it was.
    size_t state_bytes() const { return state_record_bytes(taps_, rate_) + (pk_max_ ? pk_record_bytes(rate_) : 0); }
    Status export_state(int count, const int32_t *streams, void *host_records, std::string *err);
    Status import_state(int count, const int32_t *streams, const void *host_records, std::string *err);

    // ---- output leveller: the state of the listed streams (nullptr: slots 0 .. count - 1), HOST memory float [count][2] = lvl, gain.  Runs
    // on the handle's current stream behind everything enqueued, and returns when `state` is filled (set: may be reused).  The list is
    // checked like a record list's (an index outside the handle, a slot twice: kBadArgument, nothing written); the values are the owner's
    // to check.  Stream records do not carry these eight bytes: a caller that moves a stream moves them through this pair.
    Status level_state(bool set, int count, const int32_t *streams, float *state, std::string *err);
    // ---- peak limiter: g of the listed streams, HOST memory float [count]; everything else as level_state (a handle that never limited
    // answers 1 at once and allocates nothing).  Stream records do not carry these four bytes.
    Status limiter_state(bool set, int count, const int32_t *streams, float *state, std::string *err);
    // ---- comfort noise: the frame counters of the listed streams, HOST memory uint32 [count]; everything else as level_state (a handle that
    // never filled answers 0 at once and allocates nothing).  Stream records do not carry these four bytes.
    Status comfort_state(bool set, int count, const int32_t *streams, uint32_t *n, std::string *err);

    // ---- packet handles (fourth extension).  enable_packets, once, right after create(): the handle's streams take
    // and deliver up to max_samples samples per call through run_packets; the frame entries above are then the owner's to refuse.
    bool enable_packets(int max_samples, std::string *err);
    int packet_samples() const { return pk_max_; }  // 0: a frame handle
    Status run_packets(const PacketCall &c, std::string *err);

    // ---- packet handles at 44 100 and 22 050 Hz (sixth extension).  enable_fractional, once, on a 16 kHz packet
    // engine right after enable_packets (whose max_samples is the most INNER samples a call can yield, fr_inner(max_samples) =
    // ceil(U max_samples / 441)) and before set_format: from then on run_packets takes and delivers up to max_samples samples per call at `rate`,
    // through the fractional stages (kns_fractional.hip) around the unchanged 16 kHz packet call.  Everything else of the engine stays a
    // 16 kHz packet engine's: sample_rate(), records (which the owner refuses), reports and frame counts are the inner stream's.
    bool enable_fractional(int rate, int max_samples, std::string *err);
    int fractional_rate() const { return fr_rate_; }  // 0: not such a handle

    // ---- sample formats (fifth extension).  set_format, once, right after create() -- and after enable_packets on a
    // packet handle: from then on the `pcm` and `out` of process() and run_packets() point to elements of that format (kns_kernels.h,
    // SampleFormat) behind their int16 types, sample_bytes() each, and are converted on the device around the unchanged S16 call.  The engine's
    // samples stay int16 inside: F32 is an input / output form, not a wider path.  Configuration, not stream state: records, state_bytes()
    // and the delay are those of the S16 handle.  The asynchronous host calls are refused.  kFmtS16 allocates and changes nothing.
    bool set_format(int fmt, std::string *err);
    int sample_format() const { return fmt_; }
    int sample_bytes() const { return fmt_bytes(fmt_); }

    // ---- multi-channel handles (seventh extension).  enable_channels, once, last of the enable_* / set_format calls:
    // from then on the `pcm` and `out` of process() and run_packets() are [num_streams / C][n C] elements of the handle's format -- sample i of
    // stream g C + c is element [g][i C + c] -- split into the engine's rows in front of the unchanged call and joined behind it
    // (kns_channels.hip).  Configuration, not stream state: the streams, their slots, records and every per-stream argument are those of the
    // handle without channels.  A packet call's counts must be equal within a group.  The asynchronous host calls are the owner's to refuse.
    // C == 1 allocates and changes nothing.
    bool enable_channels(int C, std::string *err);
    int channels() const { return ch_; }
    // (linked channels, StreamOptions::channel_link: a group must lie inside one 16-row mask tile)
    static bool channel_link_ok(int C) { return C == 2 || C == 4 || C == 8; }

    void profile_enable(bool on);
    bool profile_read(double *ms, int64_t *launches, std::string *err);
    int64_t debug_read(int what, float *out, int64_t capacity, std::string *err);

private:
    Engine() {}
    // The host-pointer boundary of every handle that is not the plain one (a rate other than 16 kHz, a packet handle, a sample format):
    // process() and run_packets() stage the caller's host memory in and out (kns_engine.cpp, stage_in / stage_out); everything below them
    // sees device pointers.  One staging set, allocated by the first host-pointer call: d_host_io_ [B][io_row()] elements of the handle's
    // format, the call's input and then its output; d_host_rep_ [B][Tmax][4]; and the host copies of a packet call's output and report,
    // of which only a row's first counts[b] elements and a stream's first k_b report rows go on to the caller.
    size_t io_row() const { return fr_rate_ ? (size_t) fr_max_ : pk_max_ ? (size_t) pk_max_ : (size_t) Tmax_ * rs_frame_length(rate_); }  // a stream's most elements per call
    uint8_t *d_host_io_ = nullptr;
    float *d_host_rep_ = nullptr;
    std::vector<uint8_t> host_out_;
    std::vector<float> host_rep_;
    bool stage_in(const void *pcm, size_t bytes, bool report, std::string *err);
    bool stage_out(void *out, size_t bytes, float *report, size_t report_bytes, std::string *err);
    // sample formats: the int16 staging matrices [B][io_row()] on either side of the S16 call
    int fmt_ = kFmtS16;
    int16_t *d_fmt_in_ = nullptr, *d_fmt_out_ = nullptr;
    // channels: the rows [B][io_row()] of format elements between split and join; the call below them runs on it in place
    int ch_ = 1;
    uint8_t *d_ch_ = nullptr;
    Status process_frames(const Call &c, std::string *err);  // a frame call and its held streams, below the boundary
    bool init(const Params &p, int device, int B, int Tmax, int precision, std::string *err, bool *oom);
    bool run_call(const Call &c, std::string *err);  // process() without the held streams, at 16 kHz
    // Handles that are not at 16 kHz (kns_engine.cpp, run_call_rate; device pointers): in-stage kernel, run_call on device buffers, out-stage kernel.
    // The stages' per-stream state (rs_in, rs_out: kns_kernels.h) is a ping-pong pair each, like the history; it is part of the stream
    // record (version 2), of reset() and of a call's per-frame resets.
    bool advance(const Call &c, std::string *err) { return rate_ == kRate16k ? run_call(c, err) : run_call_rate(c, err); }
    bool run_call_rate(const Call &c, std::string *err);
    // the state kernels of export / import / held streams: the engine's and, at such a rate, the stages'; packet_part: and a packet handle's
    // (not for held streams: a sub-call of a packet call does not touch the packetiser's state, whose two lengths differ inside a call)
    void launch_states(bool import, bool packet_part);
    void launch_resets(const uint8_t *d_mask);  // every reset kernel of the handle (d_mask: device [Bpad], null: every stream)
    // packet handles: the packetiser's state (kns_kernels.h, PacketArgs), the sub-calls' stacked frame matrices and reports
    // [B][Tmax F] / [B][Tmax][4], the call table (pk_up_) and the HOST MIRROR of
    // fill, from which a call is planned without a look at the device (updated by calls, resets and import_state)
    int pk_max_ = 0;
    int16_t *d_pk_pin_ = nullptr, *d_pk_pout_ = nullptr, *d_pk_in_ = nullptr, *d_pk_out_ = nullptr;
    int32_t *d_pk_fill_[2] = {nullptr, nullptr};
    float *d_pk_rep_ = nullptr;
    uint8_t *d_state_pk_ = nullptr;  // the packet part of the staged stream records [B][pk_record_bytes]
    std::vector<int32_t> pk_fill_;
    PacketStateArgs packet_state_args() const;
    // run_packets of every handle that is not a fractional one, and a fractional handle's inner call (fmt, ch: the format and the channels of
    // c.pcm / c.out -- kFmtS16 and 1 for the inner call, whose rows are the engine's)
    Status run_packet_call(const PacketCall &c, int fmt, int ch, std::string *err);
    // what the two packet calls share (kns_engine.cpp): the refusals in their order, the caller's samples onto the device and back
    struct PacketIo {
        bool host, convert;              // the caller's pointers are host memory; format kernels run (a format, and some sample)
        size_t bytes;                    // of the caller's rows that travel (0: a call without a sample)
        void *dst;                       // where the format's elements go on the device: the caller's memory or the staging
        void *joined;                    // channels: where the join writes (that memory), while dst is the rows between split and join; else nullptr
        float *report;                   // ... and the report rows, report_frames apart per stream
        int report_frames;
        const int16_t *in16;             // the int16 rows [B][max_samples] the call's first kernel reads
        int16_t *out16;                  // ... and its last one writes
    };
    Status packet_check(const PacketCall &c, int most, int ch, bool *any_restart, bool *any_count, std::string *err) const;
    Status packet_begin(const PacketCall &c, int fmt, int ch, int kmax, bool any_restart, bool any_count, PacketIo *io, bool *nothing, std::string *err);
    Status packet_end(const PacketCall &c, int fmt, int ch, const PacketIo &io, const int32_t *d_counts, const int32_t *k, int kmax, std::string *err);
    // fractional handles: the rate, the caller's max_samples, the inner path's rows [B][pk_max_] on either side of the 16 kHz packet call,
    // the stages' tables and per-stream state ([0]: in-stage, [1]: out-stage), the call table (fr_up_: int32 counts[Bpad], uint8
    // restart[Bpad]), and the HOST MIRROR of N mod 441, from which a call's inner counts are planned without a look at the device
    int fr_rate_ = 0, fr_max_ = 0;
    int16_t *d_fr_in_ = nullptr, *d_fr_out_ = nullptr, *d_fr_hist_[2] = {nullptr, nullptr};
    int32_t *d_fr_phase_[2] = {nullptr, nullptr};
    float *d_fr_taps_[2] = {nullptr, nullptr};
    std::vector<int32_t> fr_phase_;
    FractionalStateArgs fractional_state_args() const;
    Status run_fractional(const PacketCall &c, std::string *err);
    int rate_ = kRate16k;
    int16_t *d_rs_state_[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [in-stage, out-stage][ping-pong copy], [Bpad][hist] each
    int rs_cur_ = 0;
    std::vector<float> rs_taps_[2];     // the in-stage's and the out-stage's table h_U (kns_kernels.h)
    uint8_t *d_state_rs_ = nullptr;     // the stages' part of the staged stream records [B][rs_record_bytes]
    // high-band carry (Call::high_band; kns_kernels.h, HighBandArgs): the per-stream state as ping-pong pairs -- x [Bpad][hb_x_hist],
    // y [Bpad][kHbYHist], s' [Bpad][2] -- allocated (zeroed) by the first such call and part of reset(); the report [B][Tmax][4] of a call
    // whose caller asked for none; and the copy [B][Tmax F] of a call's input where its output overwrites it
    int16_t *d_hb_x_[2] = {nullptr, nullptr}, *d_hb_y_[2] = {nullptr, nullptr}, *d_hb_in_ = nullptr;
    float *d_hb_s_[2] = {nullptr, nullptr}, *d_hb_rep_ = nullptr;
    int hb_cur_ = 0;
    unsigned hb_epoch_ = 0;
    bool high_band_ready(const Call &c, std::string *err);  // the buffers, and the state cleared when the call's epoch is new
    // what run_device is given: the frames [t0, t0 + T) of a call, their device buffers, and what the call has prepared for all of its slices
    struct CallSetup;
    struct Slice {
        int t0, T;
        const int16_t *d_pcm;
        int16_t *d_out;
        bool allow_recompute;  // the synthesis kernel may rebuild the spectrum from d_pcm (false: d_out overlaps it)
        float *d_report;       // the slice's frame report [B][T][4] (device-visible memory, rows T frames apart), nullptr: not asked for
        CallSetup *call;       // begin_call's; not const: the first slice that needs the reset table uploads it
        bool without_reset_table = false;  // the captured one-frame graph: the call's other tables, but never a reset table (run_call, at the capture)
    };
    bool run_device(const Slice &s, std::string *err);
    void *dalloc(size_t bytes, bool zero);
    void *upload(const void *src, size_t bytes);
    void tick(int cls);
    void tock(int cls);

    // The immutable part of a handle -- tables and every packed weight matrix -- is built once per (model content, device, precision)
    // and SHARED by all handles that are open on it (round 6: the reference's contract is one handle per stream,
    // include/pv_koala.h:26-63; a caller with N handles used to get N folds, N packings and N weight images).  Ref-counted: freed with the
    // last handle.  A handle copies the image's pointers into its own members below; only its allocations differ.
    struct WeightImage;
    std::shared_ptr<WeightImage> weights_;
    std::vector<void *> *alloc_sink_ = nullptr;  // while an image is being built: where dalloc() records its allocations
    bool build_weights(const Params &p, int precision, std::string *err);

    int device_ = 0, B_ = 0, Bpad_ = 0, Tmax_ = 0, prec_ = 0, last_T_ = 0;
    PrecInfo pi_{};
    int nbf_ = 0, nbh_ = 0, nby_[kStages] = {0, 0, 0, 0};
    hipStream_t own_stream_ = nullptr, stream_ = nullptr;
    bool alloc_failed_ = false;
    std::vector<void *> allocs_;

    // parameters on device
    float *d_window_ = nullptr, *d_twiddle_ = nullptr, *d_mean_ = nullptr, *d_scale_ = nullptr;
    void *w_in_ = nullptr;
    float *b_in_ = nullptr;
    struct StageDev {
        void *w_ih_a, *w_hh_a, *w_ih_b, *w_hh_b, *w_head;
        float *b_ih_a, *b_hh_a, *b_ih_b, *b_hh_b, *b_head;
        int head_tiles, head_dim;
        bool ypad;  // this stage's fed-forward input rides in the padding of the features' last k-block (bf16, folded front-end, d_in <= kYPadMax)
    } sd_[kStages]{};

    // per-stream state
    int16_t *d_hist_[2] = {nullptr, nullptr};
    int hist_cur_ = 0;
    float *d_tail_[2] = {nullptr, nullptr}, *d_hstate_[2] = {nullptr, nullptr};
    void *d_hprev_ = nullptr;  // the recurrent state as A-packed operand blocks [layer][m-tile][nbh] (kRouteWave)
    int tail_cur_ = 0, hs_cur_ = 0;
    uint8_t *d_rmask_ = nullptr;
    // front-end context (front_taps > 1): features of the last front_taps - 1 frames (A-packed, one "frame" = mtiles x nbf
    // blocks), and one m-tile of the feature of a silent frame (what the context holds before a stream began)
    int taps_ = 1;
    bool fold_ = false;  // bf16, one-frame front-end: folded into the stage-input GEMMs (no front-end launch, no embedding buffer)
    void *d_fhist_ = nullptr, *d_silent_ = nullptr;
    size_t feat_frame_bytes_ = 0;

    // activation workspace (fragment layouts)
    float *d_spec_ = nullptr, *d_mask_ = nullptr;
    void *d_feat_ = nullptr, *d_e_ = nullptr, *d_y_[kStages - 1] = {nullptr, nullptr, nullptr}, *d_gi_ = nullptr,
         *d_hseq_a_ = nullptr, *d_hseq_b_ = nullptr;

    // staging for host-pointer calls: [B][Tmax * 256] each; chunked calls use them as two slots of [B][Tc * 256]
    int16_t *d_in_ = nullptr, *d_out_ = nullptr, *h_in_ = nullptr, *h_out_ = nullptr;
    // host-pointer calls with more than one sub-chunk: copy-in, compute and copy-out run on three streams
    bool process_host_pipelined(const Call &c, bool pinned, CallSetup *setup, std::string *err);
    std::vector<int> host_schedule(int T) const;  // its sub-chunk lengths
    std::vector<int> dev_host_sched_;             // developer override (KOALA_AMD_HOST_SCHED)
    // calls of several frames as a wavefront over (stage, frame): kns_engine.cpp, run_wave
    GruSmallArgs small_args(int mtb, const void *a0, int nb0, const void *a1, const void *wih, const float *bih, const void *whh,
                            const float *bhh, int layer, void *hseq, int t, const StageDev *head) const;
    GruWaveItem wave_item(int i, int t, int mtb) const;
    bool wave_fits() const;
    // mid-size batches: the (layer, chunk-of-frames) grid of a call as a wavefront over a few streams (kns_engine.cpp, run_device)
    static constexpr int kPipeStreams = 4, kPipeRing = 2;
    hipStream_t pipe_stream_[kPipeStreams] = {};
    hipEvent_t pipe_fork_ = nullptr, pipe_join_[kPipeStreams] = {}, pipe_ev_[kPipeRing][kGruLayers] = {}, pipe_syn_[kPipeRing] = {};
    bool pipe_ok_ = false, pipe_failed_ = false, dev_pipe_whole_stft_ = false;
    bool pipe_ready();
    void run_wave(int T, int mtb);
    // asynchronous host calls: two slots of full-size device staging (slot 0 = d_in_ / d_out_, slot 1 allocated on first use)
    int16_t *d_in2_ = nullptr, *d_out2_ = nullptr;
    bool async_ready_ = false;  // every event and both staging slots of the asynchronous host path exist
    hipEvent_t aev_in_[2] = {nullptr, nullptr}, aev_done_[2] = {nullptr, nullptr}, aev_out_[4] = {nullptr, nullptr, nullptr, nullptr};
    bool async_busy_[4] = {false, false, false, false};  // by call number mod 4: the window is three calls
    unsigned async_n_ = 0;
    hipStream_t copy_in_ = nullptr, copy_out_ = nullptr;
    hipEvent_t host_fork_ = nullptr;  // synchronous host calls on a caller's stream: the handle's own stream waits behind it
    hipEvent_t ev_in_[2] = {nullptr, nullptr}, ev_done_[2] = {nullptr, nullptr}, ev_out_[2] = {nullptr, nullptr};
    int host_chunk_ = 1;
    size_t host_pipeline_min_bytes_ = 0;

    // hipGraph of one host-pointer frame (copy-in, 23 kernels, copy-out); built on first use.  A captured frame has the state buffers it
    // reads and writes, and the form of its synthesis kernel, baked in: one graph per combination of the bits below
    enum FrameGraphBit {
        kGraphHidden = 1, kGraphHistory = 2, kGraphTail = 4,  // the three ping-pong indices (a one-frame call flips the hidden state only, calls of several frames in between the other two as well)
        kGraphMinGain = 8,   // an attenuation limit is in force: the kMinGain form, not the plain one
        kGraphReport = 16,   // a frame report is asked for: the kReport forms, writing to the report staging
        kGraphProfile = 32   // a band profile is in force: the kProfile forms (kGraphMinGain is set then)
    };
    int frame_graph_index(const CallSetup &s, bool report) const {  // the graph a one-frame call replays
        return hs_cur_ * kGraphHidden | hist_cur_ * kGraphHistory | tail_cur_ * kGraphTail | (s.min_gain ? kGraphMinGain : 0) | (report ? kGraphReport : 0) | (s.profile ? kGraphProfile : 0);
    }
    hipGraphExec_t frame_graph_[2 * kGraphProfile] = {};
    // completion word of the zero-copy one-frame replays (kns_stft.hip, frame_done_kernel): the host spins on a word in page-locked
    // memory instead of sleeping in hipStreamSynchronize, whose wake-up is what made p99 drift away from p50 on a busy host
    unsigned *d_frame_count_ = nullptr, *h_frame_word_ = nullptr;
    unsigned frame_seq_ = 0;
    bool frame_graph_signals_[2 * kGraphProfile] = {};
    bool spin_wait_ = true;
    bool use_graph_ = true, no_small_ = false, no_zero_copy_ = false, no_recompute_ = false, debug_taps_ = false;
    // developer switches (all read once in init() through dev_env(): compiled out of the product library)
    int dev_variant_ = 0, dev_only_class_ = -1, dev_analysis_seg_ = 0, dev_synth_seg_ = 0, dev_small_mt_ = 0, dev_steps_mt_ = 192, dev_wave_mt_ = -1, dev_wave_group_ = 0, dev_wave_parts_ = 1, dev_pipe_chunk_ = 0, dev_pipe_mt_ = -1, dev_pipe_grid_ = 0, dev_pipe_streams_ = 0;
    // one-frame calls: GRU layers fused over CU quads (kns_gruq.hip); narrow heads / front-end / mask head inside their consumers
    bool use_quad_ = true;
    int quad_nb0_max_ = 2;
    bool fuse_head_ = true, fuse_front_ = true;
    unsigned long long *d_qdbg_ = nullptr;  // developer build, KOALA_AMD_QUAD_DBG=<block>: stamps of the LAST fused launch
    int qdbg_block_ = -1;
    // the last run_device() stored the spectrum / the features / the mask (debug_read refuses a tap that was not stored)
    bool spec_valid_ = false, feat_valid_ = false, mask_valid_ = false;
    int last_head_launches_ = 0;  // recurrent launches of the last run_device() that carried their stage's head (debug tap 7)
    int last_route_ = 0;  // enum Route of the last run_device() (kns_engine.cpp; reported by the developer build's debug tap 6)
#ifdef KNS_DEV
    // frames per time segment of the last analysis / synthesis launch, and the synthesis launches of the last run_device() (one per slice
    // of the layer pipeline where the STFT stages are sliced): debug tap 6, values 4 to 6
    int last_analysis_seg_ = 0, last_synth_seg_ = 0, last_synth_launches_ = 0;
#endif

    // A table that a call sends to the device in front of its kernels: the device buffer `d` and the ring of page-locked slots that feeds it,
    // one slot per call that may still be in flight.  take() hands out the next slot for the caller to fill, once the copy that read it
    // kUploadRing takes ago has completed (an event per slot); send() enqueues the slot's copy to `d` -- or to `to` -- on `stream` and records
    // the slot's event there.  Four slots: the asynchronous window is three calls, and a device-pointer caller waits only when it is four
    // uploads ahead of the GPU.  ready(): at first use the ring, all slots or none, then `d` through dalloc, so it goes with the handle's
    // other allocations; after a failure the next call tries what is missing again.  release() frees the ring (~Engine, over uploads()).
    static constexpr int kUploadRing = 4;
    struct Upload {
        void *d = nullptr;
        void *host[kUploadRing] = {};
        hipEvent_t ev[kUploadRing] = {};
        bool pending[kUploadRing] = {};  // a copy out of the slot has been enqueued since the slot was handed out
        unsigned n = 0;
        // bytes: of a slot and of `d`; e: whose dalloc gives `d`; zero: `d` is cleared at allocation (the fractional call table only, as
        // it has always been: every other table is written whole by its first upload)
        bool ready(Engine *e, size_t bytes, bool zero = false);
        void *take(int *slot);                                   // nullptr: HIP failure
        bool send(int slot, size_t bytes, hipStream_t stream, void *to = nullptr);
        void release();
    };
    // Per-frame stream resets (kns_engine.cpp, begin_resets): a call's packed table -- per (m-tile, frame) the rows that restart, uint32
    // [mtiles][T] -- goes through rs_up_ on the stream that runs the call's kernels, a frame-0 mask through the same ring to d_rmask_.
    // The table belongs to its call: it is part of the call's CallSetup, which run_device is given with every slice.
    // rsf_up_: the sample-rate stages' copy of a call's reset flags, uint8 [B][T]; pk_up_, fr_up_: a packet call's and a fractional call's table
    Upload rs_up_, rsf_up_, pk_up_, fr_up_;
    struct ResetTable {
        int slot = -1, T = 0;        // the call's slot of rs_up_ (-1: no stream restarts after frame 0, there is no table) and its length
        bool uploaded = false;       // by the call's first run_device() that needed it
        std::vector<uint8_t> frame;  // [T]: some stream restarts at this frame of the call
    };
    bool begin_resets(int T, const uint8_t *mask, ResetTable *table, std::string *err);
    ResetArgs reset_args(const uint8_t *d_mask) const;  // the reset kernel's arguments (d_mask: device [Bpad], null: every stream)

    // stream records (export_state / import_state / held streams): the device staging buffer [B_][state_bytes()] and the stream -> record
    // table, int32 [Bpad_]
    uint64_t model_key_ = 0;  // content hash of the parameters: the key of the shared weight image, the `model hash` of a record
    uint8_t *d_state_ = nullptr;
    Upload recof_up_;
    // Per-stream settings (StreamOptions; DESIGN.md section 2, "Per-stream settings"): a feature's table [Bpad][row] and the owner's
    // revision that the device holds.  Configuration, not state: no reset, record or held stream touches a table.
    // put_table: the table of the call about to run, on the handle's stream in front of the call's kernels or graph replay -- allocated at
    // first use (`what`: the feature's name in the failure message), uploaded (rows past B: zero) when the call's revision is not the
    // table's.  A table is never zeroed at allocation: all Bpad rows are uploaded, on the call's stream, before a kernel is given the
    // pointer -- a memset on the handle's own stream would be unordered with that copy after set_stream.
    struct SettingTable {
        Upload up;
        unsigned rev = 0;
        bool valid = false;
    };
    bool table_alloc(SettingTable *t, size_t row) { return t->up.ready(this, (size_t) Bpad_ * row); }
    bool put_table(SettingTable *t, size_t row, const void *rows, unsigned rev, const char *what, std::string *err);
    SettingTable mg_tab_, pf_tab_, lv_tab_, lm_tab_, cf_tab_, cfa_tab_;  // gains, band profile, leveller, limiter, comfort settings and amplitudes
    // The output stages behind the mask, in the order they have always been checked: what a refusal calls a stage, its buffers at first use
    // and its setting tables (`rows`: the call's, nullptr: the stage is off).  refuse_stages: the first stage present is refused for `why`
    enum StageBit { kStageLevel = 1, kStageLimiter = 2, kStageComfort = 4 };
    struct OutputStage {
        unsigned bit;                    // in CallSetup::stages
        const char *name, *call, *what;  // "<name> is not ...", "<call> runs on ...", "... the buffers of <what>."
        bool carries_profile;            // its kernels carry the band profile's clamp: such a call comes with the profile (and its own tables)
        bool (Engine::*ready)(std::string *);
        unsigned StreamOptions::*rev;
        struct Table { SettingTable Engine::*tab; size_t row; const void *(*rows)(const StreamOptions &); } table[2];
        bool on(const StreamOptions &o) const { return table[0].rows(o) != nullptr; }
    };
    static const OutputStage (&output_stages())[3];
    static bool refuse_stages(const StreamOptions &o, const char *why, std::string *err);
    // What a call has prepared, once, for all of its slices: the call's mutable state below its entry
    struct CallSetup {
        ResetTable resets;
        const float *min_gain = nullptr;  // the per-stream minimum gains on the device [Bpad], nullptr: no limit in force
        const float *profile = nullptr;   // the band profile on the device [Bpad][kProfileRow], nullptr: neutral (else min_gain is not null and link is 0)
        const ComfortSetting *comfort_set = nullptr;  // comfort noise: its two tables (read beside run_comfort's counter values; then profile is not null), nullptr: off
        const float *comfort_amp = nullptr;
        int link = 0;                   // linked channels: channels() when StreamOptions::channel_link is set (then min_gain is not null), else 0
        unsigned stages = 0;            // the StageBit of every output stage that is on
        const uint8_t *ctl = nullptr;   // the stages' control rows on the device (control_rows), nullptr: no byte is set
    };
    // Fills the setup of the call about to run, before anything of it is enqueued and outside any capture: the refusals of a combination of
    // Call members (the owner's to refuse by name first; a refused call enqueues nothing), then the reset table, the setting tables and the
    // control rows, on the handle's stream in front of the call's kernels or graph replay.  device_rows: pcm / out are device memory
    bool begin_call(const Call &c, bool device_rows, CallSetup *setup, std::string *err);
    // The control rows of a call with an output stage: `hold` and the reset flags as uint8 [B][T + 1], uploaded once per call, in front of its
    // first launch that reads them, and only when some byte is set (*ctl = nullptr otherwise).  One table [B][Tmax + 1], allocated by
    // whichever stage is used first
    Upload ctl_up_;
    bool ctl_ready() { return ctl_up_.ready(this, (size_t) B_ * (Tmax_ + 1)); }
    bool control_rows(const Call &c, const uint8_t **ctl, std::string *err);
    // every Upload of the handle, for ~Engine: a new table joins this list
    std::vector<Upload *> uploads() {
        return {&rs_up_, &rsf_up_, &pk_up_, &fr_up_, &recof_up_, &ctl_up_,
                &mg_tab_.up, &pf_tab_.up, &lv_tab_.up, &lm_tab_.up, &cf_tab_.up, &cfa_tab_.up};
    }
    // Output leveller (StreamOptions::level): the state [Bpad][2], allocated fresh by the first call that levels or by level_state and part
    // of every reset; the gain pairs [B][Tmax][2]; and the report [B][Tmax][4] of a call whose caller asked for none.  run_level: the two
    // launches behind a device-pointer call's kernels, for the stages and under the control rows of the call's setup
    float *d_lv_state_ = nullptr, *d_lv_gains_ = nullptr, *d_lv_rep_ = nullptr;
    bool level_ready(std::string *err);
    bool run_level(const Call &c, const float *report, bool callers_report, const CallSetup &setup, std::string *err);
    // Peak limiter (StreamOptions::limiter): g of every stream [Bpad], allocated at 1 by the first call that limits or by limiter_state --
    // together with the leveller's buffers, whose gain pairs the limiter's launch reads -- and part of every reset.  run_level launches it in
    // level_apply_kernel's place
    float *d_lm_state_ = nullptr;
    bool limiter_ready(std::string *err);
    // Comfort noise (StreamOptions::comfort): the counters [Bpad], allocated at 0 by the first call that fills or by comfort_state and part of
    // every reset; the counter values of a call's frames [Bpad][Tmax].  run_comfort: the counter's launch in front of a device-pointer
    // call's kernels, under the control rows of the call's setup
    uint32_t *d_cf_state_ = nullptr, *d_cf_n_ = nullptr;
    bool comfort_ready(std::string *err);
    bool run_comfort(const Call &c, const CallSetup &setup, std::string *err);
    // level_state, limiter_state, comfort_state: N values of type T per stream, `fresh` on a handle that never used the stage
    template <class T, int N>
    Status stage_state(bool set, int count, const int32_t *streams, T *state, const T (&fresh)[N], T *Engine::*dev, bool (Engine::*ready)(std::string *), std::string *err);
    // a stream list (nullptr: slots 0 .. count - 1): count, range and "no slot twice"; inv [Bpad]: stream -> place in the list, -1 = not listed
    Status check_stream_list(int count, const int32_t *streams, std::vector<int32_t> *inv, std::string *err) const;
    // Frame report (Call::report) of host-pointer calls: device and page-locked host staging [B][Tmax][4] each, used like d_out_ / h_out_ (two
    // slots of [B][host_chunk_][4] by the sub-chunked calls; the one-frame graph writes into h_report_ or copies to it); d_report2_: the second
    // slot of asynchronous host calls.  Allocated by the first call that asks for a report.
    float *d_report_ = nullptr, *h_report_ = nullptr, *d_report2_ = nullptr;
    bool report_ready(bool second_slot, std::string *err);
    bool state_ready(std::string *err);
    Status state_list(int count, const int32_t *streams, std::string *err);  // checks the list, uploads its inverse table
    StateArgs state_args() const;

    // profiling
    bool profiling_ = false;
    struct Span {
        int cls;
        hipEvent_t a, b;
    };
    std::vector<Span> spans_;
    std::vector<hipEvent_t> pool_;
    hipEvent_t pending_ = nullptr;
    double acc_ms_[kNumKernelClasses] = {0, 0, 0, 0, 0};
    int64_t acc_n_[kNumKernelClasses] = {0, 0, 0, 0, 0};
};

int visible_gpu_count();
std::string gpu_name(int device);

}  // namespace kns
