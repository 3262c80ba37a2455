/*
 * pv_koala_batch.h -- additive batch extension of the Koala C ABI (SURVEY.md 8b "Batch extension").
 *
 * The reference ABI is one stream per handle, one frame per call (include/pv_koala.h:65-80); BASELINE.json's
 * configs need thousands of independent streams per GPU.  A batch handle is B streams advancing in lock step;
 * stream b of a batch behaves exactly like its own pv_koala_t (same samples, same delay, same reset semantics).
 * pv_koala_init/process are the B = 1 instance of the same engine.
 */
#ifndef PV_KOALA_BATCH_H
#define PV_KOALA_BATCH_H

#include <stdint.h>

#include "picovoice.h"
#include "pv_koala.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pv_koala_batch pv_koala_batch_t;

typedef enum {
    PV_KOALA_PRECISION_FP32 = 0, /* fp32 operands on the f32 MFMA path: +-1 LSB against the fp32 oracle       */
    PV_KOALA_PRECISION_BF16 = 1  /* bf16 GEMM operands, fp32 accumulate and gates, fp32 FFT (BASELINE configs[2]) */
} pv_koala_precision_t;

/* `device` accepts the grammar of pv_koala_init.  `max_frames_per_call` bounds `num_frames` of process_chunk and
 * sizes the activation workspace in HBM. */
PV_API pv_status_t pv_koala_batch_init(const char *access_key, const char *model_path, const char *device,
                                       int32_t num_streams, int32_t max_frames_per_call,
                                       pv_koala_precision_t precision, pv_koala_batch_t **object);
PV_API void pv_koala_batch_delete(pv_koala_batch_t *object);

/* A batch handle at a SAMPLE RATE of 8 000, 12 000, 16 000, 24 000, 32 000 or 48 000 Hz, fixed at creation (any other value:
 * PV_STATUS_INVALID_ARGUMENT).
 * 16 000 is pv_koala_batch_init's handle: same routes, launches, samples and stream records.  At the other rates a call converts the
 * streams to 16 kHz on the device, runs the 16 kHz call unchanged and converts the enhanced samples back (third
 * extension: a 48 R + 1 tap windowed-sinc low-pass, R = 2 or 3, evaluated in a fixed order; 12 000 and 24 000 go through 48 kHz in two
 * rational stages, 4/3 and 3/4 or 2/3 and 3/2, of the same low-pass with R = 4 or 3; the converters' per-stream state lives in
 * the handle, takes part in every kind of reset and in held streams, and travels in the stream record, which is version 2 then).
 *   - a frame is pv_koala_batch_frame_length() = sample_rate * 256 / 16000 samples (128 / 192 / 256 / 384 / 512 / 768 at 8 / 12 / 16 / 24 / 32 / 48 kHz:
 *     16 ms at every rate), and every
 *     entry point that advances streams takes [num_streams][num_frames * frame_length] (process, process_chunk, _resets, _hold,
 *     process_call with its frame report, whose rows are those of the inner 16 kHz stream, one per frame);
 *   - pv_koala_batch_delay_sample() is 176 / 240 / 256 / 456 / 608 / 912 samples at the handle's rate: the engine's frame and both
 *     converters (a packet handle: frame_length - 1 more, 431 at 12 kHz and 839 at 24 kHz);
 *   - host pointers: one copy in, the device route, one copy out, then synchronise; `pcm` and `enhanced` may overlap in any way, with
 *     host and with device pointers (the input is consumed before the output is written);
 *   - the asynchronous entry points, and `asynchronous != 0` in pv_koala_batch_process_call, are refused with PV_STATUS_INVALID_ARGUMENT on
 *     a handle whose rate is not 16 000 (nothing processed). */
PV_API pv_status_t pv_koala_batch_init_rate(const char *access_key, const char *model_path, const char *device,
                                            int32_t num_streams, int32_t max_frames_per_call,
                                            pv_koala_precision_t precision, int32_t sample_rate, pv_koala_batch_t **object);
PV_API pv_status_t pv_koala_batch_sample_rate(const pv_koala_batch_t *object, int32_t *sample_rate);
PV_API pv_status_t pv_koala_batch_frame_length(const pv_koala_batch_t *object, int32_t *frame_length);

/* One frame per stream: pcm and enhanced are [num_streams][256] row-major int16.  Pointers may be host memory
 * (staged through pinned buffers, call returns when `enhanced` is filled) or device memory on the handle's GPU
 * (kernels are enqueued on the handle's stream and the call returns without synchronising). */
PV_API pv_status_t pv_koala_batch_process(pv_koala_batch_t *object, const int16_t *pcm, int16_t *enhanced);

/* `num_frames` consecutive frames per stream: [num_streams][num_frames*256].  DEVICE pointers: `enhanced` may be the same
 * buffer as `pcm` (in-place) or overlap it partially (detected; the call then takes the stored-spectrum path).  HOST
 * pointers: `enhanced` may equal `pcm` EXACTLY in every call (in-place).  A PARTIAL overlap is fine while the call is not
 * pipelined in sub-chunks (below 4 MiB, or num_frames <= min(16, max_frames_per_call / 2)); larger host calls copy chunks out
 * while later chunks of `pcm` are still unread, so partially overlapping host buffers are rejected with PV_STATUS_RUNTIME_ERROR
 * (nothing is processed, the streams' state is unchanged). */
PV_API pv_status_t pv_koala_batch_process_chunk(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                int16_t *enhanced);

/* The same for a throughput-oriented host caller (a many-files batch job that double-buffers its I/O): `pcm` and `enhanced` must be
 * PAGE-LOCKED host memory (pv_koala_batch_host_alloc, hipHostMalloc, hipHostRegister; anything else is refused with
 * PV_STATUS_RUNTIME_ERROR, nothing processed).  The call enqueues its copy-in, kernels and copy-out and RETURNS; up to three such calls are
 * in flight per handle (a fourth first waits for the oldest), so one call's copies run under its neighbours' kernels -- a synchronous
 * call cannot hide its first copy-in and last copy-out.  Calls complete in order; `enhanced` of a call is valid, and `pcm` may be
 * reused, once pv_koala_batch_synchronize() or pv_koala_batch_async_wait() says the call has completed (a caller rotating over three
 * buffer pairs keeps both directions of the link and the GPU busy at once).  Every other entry
 * point of the handle first waits for the calls in flight.  `enhanced` may equal `pcm`. */
PV_API pv_status_t pv_koala_batch_process_chunk_async(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                      int16_t *enhanced);

/* pv_koala_batch_process_chunk with PER-FRAME STREAM RESETS.  `reset` is HOST memory, uint8 [num_streams][num_frames] (row-major, one
 * row per stream); NULL means no resets.  If reset[b][t] != 0, stream b is set to the fresh state (analysis history, overlap-add tail and
 * the eight GRU hidden states, as pv_koala_batch_reset would leave them) immediately before frame t of this call, and its output from
 * frame t on is exactly what a freshly reset stream produces.  A stream may reset at any number of frames of one call, adjacent ones,
 * frame 0 and frame num_frames - 1 included, so utterances shorter than a call can be packed back to back into one stream.
 * Equivalent definition: the call gives the same result as cutting it at each stream's reset frames into consecutive sub-calls with
 * pv_koala_batch_reset of exactly those streams between them -- fp32: the same samples; bf16: within the same bar as against the bf16
 * oracle.  A NULL or all-zero mask makes the call pv_koala_batch_process_chunk, route and bits.  Resets at frame 0 only are carried out
 * by the reset kernel in front of the call, which then keeps its route; resets at a later frame put the call (host calls of 4 MiB or more:
 * each sub-chunk that holds one) on the chunked kernels' reset arms at every batch size.
 * Pointers as for pv_koala_batch_process_chunk: host pointers synchronous, device pointers enqueued on the handle's stream without a host
 * wait (a caller that runs more than four such calls ahead of the GPU waits for the oldest one's mask upload).  `reset` is read before the
 * function returns.  Arguments: as pv_koala_batch_process_chunk (PV_STATUS_INVALID_ARGUMENT: NULL object / pcm / enhanced, num_frames
 * outside [1, max_frames_per_call]); in addition PV_STATUS_INVALID_ARGUMENT, with a message on the error stack, for a model with a
 * several-frame front-end (KNS-v1.1, front_taps > 1) and a non-zero reset[b][t] at any t > 0: nothing is processed and the state is
 * unchanged.
 * A corpus job (many independent files on one handle, koala_amd/corpus.py): every stream is a slot that plays one file after the other;
 * each file is laid out as ceil(samples / 256) + 1 frames (the last one a zero flush frame: delay_sample is one frame) and its first
 * frame carries the reset bit; the output of file f is its frames' output from sample delay_sample on, trimmed to its length. */
PV_API pv_status_t pv_koala_batch_process_chunk_resets(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                       int16_t *enhanced, const uint8_t *reset);

/* The same for page-locked host buffers, asynchronous: the rules of pv_koala_batch_process_chunk_async (at most three calls in flight,
 * `enhanced` valid once the call has completed).  `reset` is copied before the function returns into storage of the call's own in-flight
 * slot: the caller may overwrite it at once. */
PV_API pv_status_t pv_koala_batch_process_chunk_resets_async(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                             int16_t *enhanced, const uint8_t *reset);

/* Blocks until at most `max_in_flight` asynchronous calls of the handle are still in flight (0: all have completed; calls complete in
 * order).  The triple-buffering loop of a host caller:  for call n:  pv_koala_batch_async_wait(o, 2)  -- call n - 3 is complete: take its
 * `enhanced`, refill its `pcm` --  then pv_koala_batch_process_chunk_async(o, frames, pcm[n % 3], enhanced[n % 3]). */
PV_API pv_status_t pv_koala_batch_async_wait(pv_koala_batch_t *object, int32_t max_in_flight);

/* Resets the streams whose byte in `stream_mask[num_streams]` (host memory) is non-zero; NULL resets all. */
PV_API pv_status_t pv_koala_batch_reset(pv_koala_batch_t *object, const uint8_t *stream_mask);

/* PER-STREAM STATE AS RECORDS: move a stream to another slot, another handle (any num_streams / max_frames_per_call), another GPU or
 * another process; drain a handle for a restart; park a stream that is on hold and give its slot away.  A record is plain bytes,
 * self-contained and position-independent, little-endian, pv_koala_batch_state_size() bytes for a given model:
 *
 *     header, 32 bytes   magic "KNSS", uint32 version = 1, uint32 front_taps, uint32 precision, uint64 model content hash,
 *                        8 reserved zero bytes
 *     hist   int16[256]                  the previous frame's input samples
 *     tail   float[256]                  overlap-add tail
 *     h      float[8][271]               the eight GRU hidden vectors, layer-major (the order of debug tap 3)
 *     fctx   float[front_taps - 1][257]  the front-end's feature context, oldest frame first (KNS-v1.1 models only)
 *
 * 10 240 bytes for a model with a one-frame front-end (padded with zero bytes to a multiple of 16 for front_taps 2 ... 4).  It does not
 * depend on num_streams, the slot or anything else of the handle that wrote it.  A record belongs to one model and one precision:
 * importing it into a handle of another model, another front_taps or the OTHER PRECISION is refused (a bf16 stream does not continue
 * as an fp32 stream).
 *
 * `records` is HOST memory (pageable or page-locked), count x state_size bytes; record i belongs to stream streams[i]; streams == NULL
 * means slots 0 .. count - 1.  Both calls first wait for asynchronous host calls in flight and then run on the handle's stream, behind
 * everything enqueued on it.  Export returns when the records are filled.  Import returns when `records` may be reused, and the streams
 * continue from the imported state in the next call; a freshly created or reset stream's record imports as a reset.
 * PV_STATUS_INVALID_ARGUMENT, with a message on the error stack: NULL object / records, count outside [1, num_streams], an index outside
 * [0, num_streams), a slot listed twice, and on import any header that does not match the handle (the message names the record and the
 * field, "record 3: model hash ...").  Everything is checked before anything is written: a refused call leaves all state as it was.
 * PV_STATUS_RUNTIME_ERROR: a HIP failure.  The first such call allocates a device staging buffer of num_streams records. */
PV_API pv_status_t pv_koala_batch_state_size(const pv_koala_batch_t *object, int32_t *num_bytes);
PV_API pv_status_t pv_koala_batch_export_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, void *records);
PV_API pv_status_t pv_koala_batch_import_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams,
                                               const void *records);

/* pv_koala_batch_process_chunk with HELD STREAMS.  `hold` is HOST memory, uint8 [num_streams], read before the function returns; NULL
 * means none.  A stream with hold[b] != 0 is NOT ADVANCED by the call: afterwards its state is bit for bit what it was before, as if the
 * call had not happened for it (a live stream whose next frames have not arrived).  Its rows of `pcm` are read but meaningless, its rows
 * of `enhanced` are unspecified.  Every other stream behaves exactly as in pv_koala_batch_process_chunk.  A NULL or all-zero mask makes
 * the call pv_koala_batch_process_chunk: same route, same launches, same bits.  Otherwise the held streams' records are set aside in
 * device memory in front of the call and put back behind it -- two more launches on the handle's stream, no host wait for device
 * pointers.  Not combined with per-frame resets or the asynchronous host path. */
PV_API pv_status_t pv_koala_batch_process_chunk_hold(pv_koala_batch_t *object, int32_t num_frames, const int16_t *pcm,
                                                     int16_t *enhanced, const uint8_t *hold);

/* PER-STREAM ATTENUATION LIMIT: how hard the suppressor may bite, stream by stream.  Every stream b has a MINIMUM MASK GAIN g_b, an fp32
 * value in [0, 1]; a new handle has g_b = 0 for every stream.  In every frame processed while g_b is in force, the mask value m of each of
 * the 257 bins (DC and Nyquist included) becomes
 *
 *     m' = g_b + (1 - g_b) * m        fp32: u = 1 - g_b, then the product u * m rounded, then the sum rounded (two roundings, no fma)
 *
 * and the frame is synthesised from m' exactly as it is from m otherwise.  g = 0 is the handle without a limit (m' = m: the same samples,
 * and when EVERY stream's gain is 0 also the same route and kernels); g = 1 is a pure delay by delay_sample samples (m' = 1: the output is
 * the input, bit for bit, in both precisions, for any model) -- a bypass that keeps the stream's latency; in between no bin is attenuated by
 * more than -20 log10(g) dB: g = 0.25 is "at most 12 dB".  The mask network never sees its own output: a stream's hidden state, history and
 * feature context evolve exactly as without a limit, so the limit may be changed between any two calls without disturbing what the stream
 * has adapted to.  A change takes effect with the next call and holds for every frame of that call (the first output frame after a change
 * overlap-adds a tail made under the old gain: this is the definition, nothing is smoothed).
 * The limit is CONFIGURATION, NOT STATE: pv_koala_batch_reset, per-frame resets, held streams and export_state / import_state neither change
 * nor carry it (the stream record is unchanged); a caller that moves a stream sets its limit at the destination.  It applies to every
 * entry point that advances streams -- process, process_chunk, _async, _resets, _resets_async, _hold -- for host and device pointers alike.
 *
 * pv_koala_batch_set_min_gain: gains[i] is the minimum gain of stream streams[i]; streams == NULL means slots 0 .. count - 1; streams not
 * listed keep theirs.  Both arrays are HOST memory, read before the function returns.  No device work and no wait: the gains travel with
 * the next call (asynchronous host calls in flight keep the gains they were issued under).  PV_STATUS_INVALID_ARGUMENT, with a message
 * on the error stack and NOTHING changed: NULL object / gains, count outside [1, num_streams], an index outside [0, num_streams), a slot
 * listed twice, a gain that is NaN or outside [0, 1] (the message names the entry, "gain 3: ...").
 * pv_koala_batch_get_min_gain: the gains in force, gains[num_streams]. */
PV_API pv_status_t pv_koala_batch_set_min_gain(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const float *gains);
PV_API pv_status_t pv_koala_batch_get_min_gain(const pv_koala_batch_t *object, float *gains /*[num_streams]*/);

/* The same for the single-stream handle of pv_koala.h (an extension: the reference library has no such control): the limit of
 * pv_koala_process from the next frame on.  PV_STATUS_INVALID_ARGUMENT for a NULL argument, a NaN or a gain outside [0, 1]. */
PV_API pv_status_t pv_koala_set_min_gain(pv_koala_t *object, float gain);
PV_API pv_status_t pv_koala_get_min_gain(const pv_koala_t *object, float *gain);

/* FRAME REPORT: what the suppressor did to every stream in every frame -- for voice activity and talker detection, for a "this caller is
 * being gated to nothing" alarm (the moment to raise pv_koala_batch_set_min_gain), for per-file figures of a corpus job.  Four fp32 values per
 * stream and frame, formed by the synthesis kernel from what it holds anyway (fixes every operation and the
 * summation order; fp32 handles are bit-exact against it):
 *
 *     report[b][t][0]  e_in      sum over the 257 bins of |X[k]|^2, X the spectrum of the 512-sample analysis block whose second half is
 *                                input frame t (sqrt-Hann window, samples / 32768)
 *     report[b][t][1]  e_out     the same sum over Y[k] = m'[k] X[k], the spectrum that is synthesised (m': the mask under the stream's
 *                                attenuation limit)
 *     report[b][t][2]  mask_sum  sum of the network's RAW mask m[k] (before the attenuation limit: the speech cue does not depend on a
 *                                tenant's limit); mask_sum / 257 is the mean gain the model asked for
 *     report[b][t][3]  reserved, 0
 *
 * The block of report row t leaves as output frame t (its first half, overlap-added).  Exact in both precisions: a stream with minimum
 * gain 1 has e_out == e_in; a block of digital silence reports zeros; in a reset frame the report is that of the block [0 | frame t].  The
 * report is an output only: samples and stream state are bit for bit the same whether or not it is asked for, and a call that does not ask
 * runs the kernels it always ran.  Held streams' rows are unspecified.  koala_amd/report.py turns rows into dBFS, suppression in dB and
 * mean gain.
 *
 * pv_koala_batch_process_call: ONE entry point for every way of advancing the streams; the members select what the dedicated entry points
 * select.  With report == NULL the call is exactly the existing entry point its other members name -- pv_koala_batch_process_chunk,
 * _async, _resets, _resets_async or _hold: same route, same bits.  `report` is memory of the same kind as `enhanced` (host with host,
 * device with device; asynchronous calls: page-locked, valid once the call has completed) -- anything else is PV_STATUS_RUNTIME_ERROR like
 * the other pointer-kind refusals.  PV_STATUS_INVALID_ARGUMENT, with a message on the error stack and nothing processed: a NULL object /
 * call / pcm / enhanced, num_frames outside [1, max_frames_per_call], a struct_size that is not sizeof(pv_koala_batch_call_t), hold together
 * with reset, hold together with asynchronous, and a KNS-v1.1 model with a reset at a frame t > 0. */
typedef struct {
    int32_t struct_size;      /* sizeof(pv_koala_batch_call_t): lets the struct grow */
    int32_t num_frames;
    const int16_t *pcm;       /* [num_streams][num_frames * 256] */
    int16_t *enhanced;        /* [num_streams][num_frames * 256] */
    const uint8_t *reset;     /* [num_streams][num_frames] or NULL (pv_koala_batch_process_chunk_resets) */
    const uint8_t *hold;      /* [num_streams] or NULL (pv_koala_batch_process_chunk_hold) */
    float *report;            /* [num_streams][num_frames][4] or NULL */
    int32_t asynchronous;     /* non-zero: the rules of pv_koala_batch_process_chunk_async */
} pv_koala_batch_call_t;
PV_API pv_status_t pv_koala_batch_process_call(pv_koala_batch_t *object, const pv_koala_batch_call_t *call);

/* pv_koala_process of the single-stream handle of pv_koala.h with the frame's report (an extension: the reference library has no such
 * call).  Calls with and without a report may be mixed freely: the samples are those of a handle that never asked. */
PV_API pv_status_t pv_koala_process_report(pv_koala_t *object, const int16_t *pcm, int16_t *enhanced_pcm, float report[4]);

/* PACKET HANDLES: streams that deliver ANY NUMBER OF SAMPLES per call.  Live audio arrives in 10 and 20 ms packets (80 / 160 / 320 / 480 /
 * 960 samples), with jitter and not in phase across callers; a packet handle is a batch handle at any of the six rates whose streams are
 * sample-in / sample-out filters (fourth extension).  With F the frame length, D the frame handle's delay_sample at
 * that rate, x everything stream b was given since its last reset and e what a frame handle produces for x cut into frames, the stream's
 * output is  o = [F - 1 zeros] ++ e,  and every call delivers the next counts[b] samples of it: pv_koala_batch_delay_sample() is D + F - 1
 * (511 at 16 kHz).  The handle rebuffers on the device in both directions, so device pointers stay device pointers and no host loop
 * runs per stream.
 *   - pv_koala_batch_init_packets: `max_samples_per_call` >= 1 bounds `max_samples` of a call; the engine behind the handle is made
 *     with max_frames_per_call = ceil(max_samples_per_call / F).
 *   - the frame entry points (process, process_chunk*, process_call, the asynchronous ones) are refused on a packet handle, and
 *     pv_koala_batch_process_packets on a frame handle, with PV_STATUS_INVALID_ARGUMENT, a message on the error stack and nothing processed.
 *   - per-stream state on top of the frame handle's: fill = (length of x) mod F and one buffer of F - 1 int16 whose first `fill` entries
 *     are pending input and whose last F - 1 - fill entries are pending output.  Every reset (pv_koala_batch_reset, full or masked, and
 *     `restart`) makes it fill = 0 and F - 1 zeros.  It travels in the stream record, which is VERSION 3 then: the header with its version
 *     and sample_rate fields set, the handle's version 1 or 2 body, uint32 fill, int16[F - 1], zero-padded to whole 16-byte words.  A packet
 *     handle writes and accepts version 3 of its own rate only; a stream parked or moved mid-frame continues sample for sample.
 *
 * pv_koala_batch_process_packets: stream b gives its next counts[b] samples and takes the next counts[b] samples of its output.
 * counts[b] = 0 is a stalled stream: it is not advanced, bit for bit (this replaces `hold`).  `pcm` and `enhanced` are host memory (the
 * call is synchronous) or device memory (the call is enqueued on the handle's stream with no host wait) and may overlap in any way: the
 * input is consumed before the output is written.  `counts`, `restart` and `frames` are always HOST memory; the first two are read and
 * `frames` is written before the function returns.  Stream b completes k_b = floor((fill_b + counts[b]) / F) frames in the call:
 * frames[b] = k_b, and report[b][0 .. k_b) are those frames' report rows (rows past k_b are unspecified).  The attenuation limit applies
 * unchanged.  PV_STATUS_INVALID_ARGUMENT, with a message on the error stack and all state unchanged: a NULL object / call / counts / pcm /
 * enhanced, a struct_size that is not sizeof(pv_koala_batch_packets_t), max_samples outside [1, max_samples_per_call], a count outside
 * [0, max_samples], a report with report_frames below the largest k_b of the call, `pcm` in host and `enhanced` in device memory or the
 * other way round, a `report` that is not memory of enhanced's kind. */
PV_API pv_status_t pv_koala_batch_init_packets(const char *access_key, const char *model_path, const char *device, int32_t num_streams,
                                               int32_t max_samples_per_call, pv_koala_precision_t precision, int32_t sample_rate,
                                               pv_koala_batch_t **object);
PV_API pv_status_t pv_koala_batch_is_packet_handle(const pv_koala_batch_t *object, int32_t *is_packet_handle);
typedef struct {
    int32_t struct_size;      /* sizeof(pv_koala_batch_packets_t): lets the struct grow */
    int32_t max_samples;      /* row length of pcm / enhanced, 1 .. max_samples_per_call */
    const int32_t *counts;    /* HOST [num_streams], each in [0, max_samples] */
    const int16_t *pcm;       /* [num_streams][max_samples], row b's first counts[b] samples count */
    int16_t *enhanced;        /* [num_streams][max_samples], row b's first counts[b] samples are written */
    const uint8_t *restart;   /* HOST [num_streams] or NULL: the stream is fresh before this packet (a join) */
    float *report;            /* [num_streams][report_frames][4] or NULL, memory of enhanced's kind */
    int32_t report_frames;    /* rows per stream of `report`: at least the most frames any stream completes in the call */
    int32_t *frames;          /* HOST [num_streams] or NULL, out: the frames stream b completed in this call */
} pv_koala_batch_packets_t;
PV_API pv_status_t pv_koala_batch_process_packets(pv_koala_batch_t *object, const pv_koala_batch_packets_t *call);

/* SAMPLE FORMATS: batch handles that take and deliver float32 or G.711 samples, converted on the device.  Telephony holds 8 kHz G.711, one
 * byte per sample; WebRTC and everything that arrives as a tensor holds float32 in [-1, 1).  A batch handle has a sample format, fixed at
 * creation and orthogonal to its rate and to frame / packet kind (fifth extension):
 *   PV_KOALA_SAMPLE_S16   int16   the handle as it has always been
 *   PV_KOALA_SAMPLE_F32   float   in: NaN -> 0, else x * 32768 rounded half away from zero and clipped to [-32768, 32767]; out: s / 32768
 *   PV_KOALA_SAMPLE_ULAW  uint8   ITU G.711 mu-law on a 16-bit scale (255 levels in +-32124; the encoder truncates; 0x7F decodes to 0 and
 *                                 0 encodes to 0xFF)
 *   PV_KOALA_SAMPLE_ALAW  uint8   ITU G.711 A-law on a 16-bit scale (256 levels in +-32256; the encoder truncates)
 * A call of such a handle is: decode every sample the call reads -> the S16 handle's call, unchanged -> encode every sample the call
 * writes.  So its output is exactly encode(S16 handle(decode(input))) in both precisions, and everything else a handle does -- rates,
 * frame report (rows of the decoded stream), attenuation limit, resets of every kind, held streams, packet calls with stalled and
 * restarting streams -- is the S16 handle's.  The engine's samples stay int16 inside: F32 is an input / output form, not a wider path
 * (for inputs s / 32768 an F32 handle is the S16 handle value for value).  The format is CONFIGURATION of the handle, not stream state:
 * delay_sample and frame_length (in samples), state_size and the stream record (version and bytes) are the S16 handle's, and a record
 * written by a handle of one format imports into a handle of another that matches in model, precision, rate and kind.  A packet handle's
 * leading F - 1 output zeros are encode(0): 0.0f, 0xFF, 0xD5.
 *
 * pv_koala_batch_init_config is the one constructor for every kind of batch handle.  With PV_KOALA_SAMPLE_S16 the handle is exactly what
 * pv_koala_batch_init / _init_rate / _init_packets returns for the other members.  PV_STATUS_INVALID_ARGUMENT with a message on the
 * error stack: a NULL config, a struct_size that is not sizeof(pv_koala_batch_config_t), a sample_format outside 0 ... 3, and whatever
 * the three constructors refuse.
 *
 * PACKET HANDLES AT 44 100 AND 22 050 Hz are reached through this constructor alone, with max_samples_per_call in [1, 4 194 304]
 * (pv_koala_batch_init_rate and _init_packets keep refusing the two rates; max_samples_per_call == 0 is refused with a message that names
 * `sample_rate`: 16 ms is not a whole number of samples there, so such a handle must be a packet handle).  16 000 / rate is 160 / 441 or
 * 320 / 441: the handle converts on the device on either side of the unchanged 16 kHz packet path (sixth extension).
 * Sample in, sample out like every packet handle: a call delivers row b's next counts[b] samples, pv_koala_batch_delay_sample later --
 * 1541 at 44 100 Hz, 771 at 22 050 Hz.  Report rows and frames[b] are those of the inner 16 kHz stream (16 ms frames of 256 samples at
 * 16 kHz: a stream that is given n samples completes about n * 16000 / rate / 256 of them; report_frames follows that).  restart,
 * pv_koala_batch_reset, the attenuation limit, sample formats, host and device pointers and overlapping pcm / enhanced work as on the
 * other packet handles; pv_koala_batch_sample_rate, _delay_sample, _is_packet_handle and _sample_format answer as usual.
 * pv_koala_batch_frame_length returns PV_STATUS_INVALID_ARGUMENT with a message: there is no whole frame.  NOT YET at these rates, each
 * refused with PV_STATUS_INVALID_ARGUMENT and a message, nothing processed: stream records (pv_koala_batch_state_size, _export_state,
 * _import_state), the asynchronous entry points (with every frame entry point: the handle is a packet handle), and 11 025 Hz.
 *
 * THE PROCESSING ENTRY POINTS KEEP THEIR SIGNATURES (there are no void* twins).  On a handle with a format, every `pcm` and `enhanced` --
 * of pv_koala_batch_process, _process_chunk, _resets, _hold, _process_call and _process_packets -- points to elements of the handle's
 * format behind its int16_t type: float[...] or uint8_t[...] of the documented shape, cast by the caller.  A device pointer need be
 * aligned to its element only.  Host pointers: one copy in of the format's bytes, the device route, one copy out, then synchronise;
 * `pcm` and `enhanced` may overlap in any way, with host and with device pointers (every extent is in bytes of the format; the input is
 * consumed before the output is written).  A packet call writes row b's first counts[b] elements only.  pv_koala_batch_host_alloc takes
 * bytes: num_streams * samples * (4, 1 or 1).  The asynchronous entry points, and `asynchronous != 0` in pv_koala_batch_process_call, are
 * refused with PV_STATUS_INVALID_ARGUMENT on a handle whose format is not S16 (nothing processed).  The single-stream ABI (pv_koala.h)
 * is int16 only. */
typedef enum {
    PV_KOALA_SAMPLE_S16 = 0,
    PV_KOALA_SAMPLE_F32 = 1,
    PV_KOALA_SAMPLE_ULAW = 2,
    PV_KOALA_SAMPLE_ALAW = 3
} pv_koala_sample_format_t;
typedef struct {
    int32_t struct_size;           /* sizeof(pv_koala_batch_config_t): lets the struct grow */
    int32_t num_streams;
    int32_t max_frames_per_call;   /* frame handles; ignored when max_samples_per_call > 0 */
    int32_t max_samples_per_call;  /* > 0: a packet handle */
    int32_t precision;             /* pv_koala_precision_t */
    int32_t sample_rate;           /* 8000 / 12000 / 16000 / 24000 / 32000 / 48000; packet handles also 22050 / 44100 */
    int32_t sample_format;         /* pv_koala_sample_format_t */
} pv_koala_batch_config_t;
PV_API pv_status_t pv_koala_batch_init_config(const char *access_key, const char *model_path, const char *device,
                                              const pv_koala_batch_config_t *config, pv_koala_batch_t **object);
PV_API pv_status_t pv_koala_batch_sample_format(const pv_koala_batch_t *object, int32_t *sample_format);

/* CHANNELS: batch handles whose `pcm` and `enhanced` hold several streams interleaved, split and joined on the device.  Stereo and
 * multi-microphone audio arrives interleaved (L R L R ...) from WebRTC, Opus and WAV.  `channels` is the MEMORY LAYOUT of `pcm` and
 * `enhanced` and nothing else; it sits at the same boundary as the sample format, outside it (seventh extension).
 * A handle with channels = C (2 ... 8) and num_streams = B has G = B / C groups; stream s = g * C + c is channel c of group g -- an
 * ordinary, independent stream of the engine, with the slot, the state and the record it has in a handle made without channels.
 *   Layout.  Every `pcm` and `enhanced` is [G][n * C] elements of the handle's sample format, n = a stream's row length in the handle
 *     without channels (num_frames * frame_length, or max_samples of a packet call): sample i of stream g * C + c is element
 *     [g][i * C + c].
 *   Output.  Exactly interleave(the handle without channels(deinterleave(pcm))), given the same per-stream arguments: every rate, frame
 *     and packet handles, every format, both precisions.
 *   Per-stream arguments stay per stream, [B], indexed by s: reset[B][T], hold[B], the streams of pv_koala_batch_set_min_gain,
 *     report[B][T][4], counts[B], restart[B], frames[B], stream lists and records.
 *   Configuration, not stream state: state_size, the record's version and bytes are unchanged, and a record moves between handles of any
 *     channel count that match as they must today.  pv_koala_batch_delay_sample and _frame_length are in samples per channel, unchanged;
 *     pv_koala_batch_num_streams stays B.
 *   Packet calls.  The streams of a group share a row, so `counts` must be equal within a group: otherwise PV_STATUS_INVALID_ARGUMENT with a
 *     message that names the group and the two streams, nothing processed, state unchanged.  `restart` may differ within a group.  The call
 *     writes group row g's first counts[g * C] * C elements and nothing behind them.
 *   Held streams.  A held stream's elements of `enhanced` are unspecified, as its row is today; its state is untouched, bit for bit.
 *   Pointers.  `pcm` and `enhanced` may overlap in any way, with host and with device pointers: the input is consumed before the output is
 *     written.  Host pointers: one copy in, the device route, one copy out, then synchronise.  Device pointers stay device pointers,
 *     enqueued without a host wait, aligned to the element only.
 * pv_koala_batch_init_channels is pv_koala_batch_init_config with that one more argument (the struct does not grow).  channels == 1 is
 * exactly pv_koala_batch_init_config: the same handle, routes and bits.  PV_STATUS_INVALID_ARGUMENT with a message that names `channels`:
 * channels outside [1, 8], and num_streams that is not a multiple of channels; whatever pv_koala_batch_init_config refuses stays refused
 * with its own message.  The asynchronous entry points, and `asynchronous != 0` in pv_koala_batch_process_call, are refused with
 * PV_STATUS_INVALID_ARGUMENT on a handle whose channels is not 1 (nothing processed).
 * NOT PROVIDED: a planar / interleaved conversion for the single-stream ABI (pv_koala.h is one channel only). */
PV_API pv_status_t pv_koala_batch_init_channels(const char *access_key, const char *model_path, const char *device,
                                                const pv_koala_batch_config_t *config, int32_t channels,
                                                pv_koala_batch_t **object);
PV_API pv_status_t pv_koala_batch_channels(const pv_koala_batch_t *object, int32_t *channels);

/* LINKED CHANNELS: one mask per group (eighth extension).  The channels of a group are independent streams: each gets
 * its own mask, so one spectral bin is attenuated by different amounts in L and R, frame by frame, which moves the stereo image.  With the
 * link on, the mask applied to bin k of stream g * C + c in a frame is
 *     m_link[k] = max over c' in 0 .. C - 1 of m[g * C + c'][k],
 * m the network's raw mask of that frame, all 257 bins: a bin is kept in every channel if any channel holds speech there.  A max of finite
 * values: exact in both precisions, whatever the order.  Everything behind it is unchanged: the attenuation limit is applied per stream to
 * m_link (m' = g_s + (1 - g_s) m_link) and Y = m' X is synthesised as ever.
 *   State.  The network never sees its own output: a linked handle's hidden states, history, feature context and stream records evolve bit
 *     for bit as the unlinked handle's; only the overlap-add tail and the samples differ.  The link is configuration, not state: no reset,
 *     held call or record carries it, and state_size is unchanged.
 *   Frame report.  mask_sum stays the stream's own raw mask (the speech cue is per channel) and e_in is unchanged: both equal the unlinked
 *     handle's bit for bit; e_out is of the linked m'.
 *   Identical channels.  A group whose channels carry the same samples and equal state gives exactly the unlinked output.
 *   Every rate, frame and packet handles, every sample format, both precisions: interleave(linked(deinterleave(pcm))) as above.
 * pv_koala_batch_set_channel_link: per handle; may change between any two calls and takes effect with the next call, like
 * pv_koala_batch_set_min_gain; no device work and no wait.  With PV_KOALA_CHANNEL_LINK_NONE the handle is exactly the handle it was: same
 * routes, kernels and bits.  PV_STATUS_INVALID_ARGUMENT with a message, everything unchanged: a NULL object or out-pointer; a link outside
 * 0 ... 1; PV_KOALA_CHANNEL_LINK_MAX on a handle whose `channels` is not 2, 4 or 8 (the message names `channels`: a group must lie inside
 * one 16-row mask tile, so 1, 3, 5, 6 and 7 are refused).  LINK_NONE is accepted on every handle.
 * A LINKED CALL is refused with PV_STATUS_INVALID_ARGUMENT, nothing processed and state unchanged, with a message that names the group and
 * the two streams, when
 *   `hold` differs within a group (a held stream is computed on meaningless input: its mask must not reach its partner);
 *   `restart` differs within a group, in a packet call;
 *   a group is out of phase in a packet call: its streams hold different numbers of samples of an unfinished frame (at 44 100 / 22 050 Hz
 *     their positions in the 441-sample period count too).  That can follow a masked pv_koala_batch_reset or an import_state of one channel,
 *     which stay legal per stream; a reset or import of the whole group cures it.
 * Per-frame `reset` may differ within a group: the fresh stream's mask is simply what it is. */
typedef enum { PV_KOALA_CHANNEL_LINK_NONE = 0, PV_KOALA_CHANNEL_LINK_MAX = 1 } pv_koala_channel_link_t;
PV_API pv_status_t pv_koala_batch_set_channel_link(pv_koala_batch_t *object, int32_t link);
PV_API pv_status_t pv_koala_batch_get_channel_link(const pv_koala_batch_t *object, int32_t *link);

/* HIGH-BAND CARRY (ninth extension).  A frame handle at 32 000 or 48 000 Hz decimates to 16 kHz, enhances there and
 * interpolates back; both converters are the same low-pass, so nothing above about 7.5 kHz comes out of it.  With
 * PV_KOALA_HIGH_BAND_CARRY the handle adds that band back, as band-split suppressors do: with R = sample_rate / 16000 and
 * D = delay_sample (608 / 912),
 *     hb[n]  = x[n - D] - Lf[n]                      Lf: the handle's result with the engine replaced by a pure delay of one frame, kept as float
 *     out[n] = to_pcm(fmaf(G[n], hb[n], E[n]))       E: what the handle delivers without the feature
 *     G[n]   = s'[t-1] + w (s'[t] - s'[t-1])         j = floor((n - 24 R) / R), t = floor(j / 256), w = (j - 256 t) / 256
 *     s'[t]  = g + (1 - g) mask_sum[t] / 257         the frame report's mask_sum, the stream's attenuation limit g; 0 in front of the stream
 * (linked channels: the max of mask_sum over the group).  The ramp G is the overlap-add's own cross-fade.  With min_gain = 1 the whole handle
 * is a pure delay to within 1 LSB (from its third frame on, wherever Lf does not clip); a stream with no energy above the converters' pass
 * band is practically unchanged.  The mask network, E, the streams' state, the records' content and the frame report are bit for bit the
 * handle's without the feature.  koala_amd/highband.py states the rule in numpy.
 *   State: the feature keeps the last D input samples, 304 converter samples and two gains per stream, only while it is on; cleared by
 *     pv_koala_batch_reset (all or masked), by a `reset` at frame 0, and by turning the feature on: the high band is then that of streams
 *     that began with the next call.
 * pv_koala_batch_set_high_band: per handle; may change between any two calls and takes effect with the next call; no device work and no
 * wait.  With PV_KOALA_HIGH_BAND_NONE the handle is exactly the handle it was: same launches, same bits; NONE is accepted on every handle.
 * PV_STATUS_INVALID_ARGUMENT with a message, everything unchanged: a NULL object or out-pointer; a mode outside 0 ... 1; CARRY on a handle
 * whose `sample_rate` is not 32000 or 48000 (the message names `sample_rate`: 16 kHz and below have no band to carry; 24 kHz and
 * 44 100 / 22 050 Hz are not available yet); CARRY on a packet handle (not yet).
 * WHILE CARRY IS ON these are refused with PV_STATUS_INVALID_ARGUMENT, by name, nothing processed and state unchanged (not yet): a per-frame
 * `reset` at a frame behind frame 0; `hold`; pv_koala_batch_state_size, _export_state and _import_state (a record would need the feature's
 * state).  The asynchronous entry points are refused at these rates anyway. */
typedef enum { PV_KOALA_HIGH_BAND_NONE = 0, PV_KOALA_HIGH_BAND_CARRY = 1 } pv_koala_high_band_t;
PV_API pv_status_t pv_koala_batch_set_high_band(pv_koala_batch_t *object, int32_t mode);
PV_API pv_status_t pv_koala_batch_get_high_band(const pv_koala_batch_t *object, int32_t *mode);

/* BAND PROFILE (tenth extension): a floor and a ceiling on the mask per stream and per bin -- "at most 6 dB below
 * 300 Hz", "leave 4-8 kHz alone" (floors); a high-pass under the speech band, the 300-3400 Hz limit in front of a G.711 trunk (ceilings).
 * Every stream b has two curves of PV_KOALA_NUM_BINS = 257 fp32 values, bins 0 (DC) to 256 (Nyquist of the 16 kHz inner stream), 31.25 Hz
 * apart: floor_b[k] and ceil_b[k], each in [0, 1], floor_b[k] <= ceil_b[k].  A new handle has floor = 0 and ceil = 1 everywhere, the
 * NEUTRAL profile.  In every frame processed while a profile is in force, with m[k] the network's mask and g_b the stream's attenuation limit:
 *     m1[k] = g_b + (1 - g_b) m[k]                      exactly as pv_koala_batch_set_min_gain states it
 *     m'[k] = min(ceil_b[k], max(floor_b[k], m1[k]))    max first, then min; both exact
 *     Y[k]  = m'[k] X[k]
 * so the rule adds no rounding: an fp32 handle stays bit-exact against the oracle under it (koala_amd/bands.py states it in numpy).
 *   Neutral profile: the same samples; with every stream neutral the handle takes the routes and kernels it always took.
 *   floor = ceil = 1 on all bins: a pure delay by delay_sample, bit for bit, both precisions, any model.
 *   ceil = 0 on all bins: e_out == 0 in every frame, digital silence once the last frame made under the old profile has left the overlap.
 *   The network never sees its own output: stream state, records, e_in and mask_sum of the frame report are bit for bit those of the handle
 *     without a profile; e_out is that of m'.
 *   Configuration, not state: no reset, held call or record changes or carries it, and state_size is unchanged.
 * pv_koala_batch_set_band_profile: floor[i] / ceil[i] (rows of 257) are the curves of stream streams[i]; streams == NULL means slots
 * 0 .. count - 1; floor == NULL means zeros, ceil == NULL means ones; streams not listed keep theirs.  All arrays are HOST memory, read before
 * the function returns.  No device work and no wait: the table travels with the next call and is uploaded only when it has changed
 * (asynchronous host calls in flight keep the profile they were issued under).  PV_STATUS_INVALID_ARGUMENT, with a message on the error stack
 * and NOTHING changed: a NULL object, count outside [1, num_streams], an index outside [0, num_streams), a slot listed twice, a value that
 * is NaN or outside [0, 1], floor[k] > ceil[k] (the message names the entry and the bin, "profile 3, bin 17: ...").
 * pv_koala_batch_get_band_profile: the curves in force of one stream (either out-pointer may be NULL).
 * NOT YET, refused by name with PV_STATUS_INVALID_ARGUMENT, nothing processed and state unchanged: a call under a profile that is not neutral
 * on a handle whose channel link is on, or whose high-band carry is on (its broadband gain would have to follow the profile). */
#define PV_KOALA_NUM_BINS 257
PV_API pv_status_t pv_koala_batch_set_band_profile(pv_koala_batch_t *object, int32_t count, const int32_t *streams,
                                                   const float *floor /*[count][257] or NULL*/, const float *ceil /*[count][257] or NULL*/);
PV_API pv_status_t pv_koala_batch_get_band_profile(const pv_koala_batch_t *object, int32_t stream, float *floor /*[257] or NULL*/,
                                                   float *ceil /*[257] or NULL*/);
/* The same for the single-stream handle of pv_koala.h: the profile of pv_koala_process from the next frame on. */
PV_API pv_status_t pv_koala_set_band_profile(pv_koala_t *object, const float *floor /*[257] or NULL*/, const float *ceil /*[257] or NULL*/);
PV_API pv_status_t pv_koala_get_band_profile(const pv_koala_t *object, float *floor /*[257] or NULL*/, float *ceil /*[257] or NULL*/);

/* OUTPUT LEVELLER (eleventh extension): a per-stream automatic gain behind the suppressor that adapts only on frames
 * the network passed as speech, so it never pumps the noise floor back up.  It works on the samples E of the inner 16 kHz call, on the
 * device, directly behind it: every rate, sample format, channel layout and packet handle gets it.  Per stream b there is a SETTING
 * (pv_koala_level_t; a new handle: off) and two fp32 values of STATE, lvl (the tracked speech energy) and gain; fresh: lvl = 0, gain = 1.
 * For every frame t a levelling stream completes, with e_out and mask_sum of its frame report row (FRAME REPORT above), all in fp32, one
 * rounding per operation, the division and the square root correctly rounded:
 *     speech = mask_sum * (1/257) >= theta  and  e_out > e_floor
 *     if speech:  lvl = e_out if lvl == 0, else lvl + a * (e_out - lvl),  a = a_up if e_out > lvl else a_down
 *     want   = 1 if lvl == 0, else min(max_boost, max(max_cut, sqrt(target / lvl)))
 *     g_t    = gain + slew * (want - gain);  gain = g_t
 *     out[256 t + n] = to_pcm(E[256 t + n] * fmaf(n / 256, g_t - g_{t-1}, g_{t-1}))     n = 0 .. 255
 * to_pcm rounds half away from zero and saturates; what keeps a levelled stream from clipping is the PEAK LIMITER below (off on a new handle: without it, choose max_boost and
 * target with headroom).  e_out is
 * an energy in the report's units: a stationary signal of RMS r (full scale = 1) reads 65536 r^2 (koala_amd/level.py, settings(), turns dBFS
 * and milliseconds into the fields).  g_t is written to column 3 of the stream's report rows (0 for every other stream and handle).
 *   - a per-frame `reset` at frame t, a packet call's `restart` and pv_koala_batch_reset make the state fresh before that frame: its ramp
 *     starts from 1 (a per-frame `reset` of a stream whose leveller is off leaves the state alone, like every call does).
 *     A stream that is switched off and on again continues from the state it was switched off with -- its first sample is under the old
 *     gain, a step from 1 -- unless the caller sets (0, 1) with pv_koala_batch_set_level_state or resets the stream with pv_koala_batch_reset;
 *   - a held stream (`hold`, a stalled stream of a packet call) keeps its state bit for bit;
 *   - a stream whose leveller is off delivers E bit for bit and its state does not move; a handle on which no stream levels runs the
 *     launches it always ran;
 *   - the setting is configuration, like the attenuation limit: no reset, hold or record changes or carries it.  Stream records do not
 *     change either (state_size, version, bytes): the two floats travel through pv_koala_batch_get_level_state / _set_level_state, eight
 *     more bytes for a caller that moves a stream;
 *   - host pointers on a plain 16 kHz handle: while some stream levels a call is one copy in, the device route, one copy out.
 * pv_koala_batch_set_level: settings[i] is the setting of stream streams[i] (streams == NULL: slots 0 .. count - 1; streams not listed
 * keep theirs).  `struct_size` of settings[0] is the distance between the entries: sizeof(pv_koala_level_t), or more from a caller built
 * against a later header (the fields known here are read).  Everything is checked before anything changes; PV_STATUS_INVALID_ARGUMENT
 * with a message that names the entry and the field ("setting 3: `max_cut` ..."): target not > 0, max_boost not >= 1, max_cut not in (0, 1],
 * theta not in [0, 1], e_floor not >= 0, a_up / a_down / slew not in (0, 1], NaN or infinite anywhere, `on` not 0 or 1, a bad count, index
 * or struct_size.  No device work and no wait: the table travels with the next call and is uploaded only when it has changed.
 * pv_koala_batch_get_level: the caller sets setting->struct_size (sizeof(pv_koala_level_t) or more); the fields known here are written, nothing
 * behind them.
 * pv_koala_batch_get_level_state / _set_level_state: state[i] = {lvl, gain} of stream streams[i], HOST memory; they run on the handle's
 * stream behind everything enqueued and return when done (a handle that never levelled answers (0, 1) at once and allocates nothing).  An index
 * outside [0, num_streams) or a slot listed twice is refused, in either call.  Setting (0, 1) makes a stream fresh; lvl < 0, gain <= 0, NaN or infinity is refused.
 * NOT YET, refused by name with PV_STATUS_INVALID_ARGUMENT, nothing processed and state unchanged, while some stream's leveller is on: a
 * call with the channel link on (a group needs one gain), with the high-band carry on (its band would need the same gain), through the
 * asynchronous entry points, or on a handle at 44 100 / 22 050 Hz. */
typedef struct {
    int32_t struct_size; /* sizeof(pv_koala_level_t) */
    int32_t on;          /* 0: off (the other fields are kept but unused), 1: on */
    float target;        /* the energy the stream's speech frames are brought to, in the report's units, > 0 */
    float max_boost;     /* largest gain, >= 1 */
    float max_cut;       /* smallest gain, in (0, 1] */
    float theta;         /* a frame is speech when its mean mask is at least this, in [0, 1] */
    float e_floor;       /* ... and its e_out is above this, >= 0 */
    float a_up;          /* one-pole coefficient of lvl per frame when the energy rises, in (0, 1] */
    float a_down;        /* ... when it falls, in (0, 1] */
    float slew;          /* one-pole coefficient of the gain per frame, in (0, 1] */
} pv_koala_level_t;
PV_API pv_status_t pv_koala_batch_set_level(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const pv_koala_level_t *settings);
PV_API pv_status_t pv_koala_batch_get_level(const pv_koala_batch_t *object, int32_t stream, pv_koala_level_t *setting);
PV_API pv_status_t pv_koala_batch_get_level_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, float *state /*[count][2]*/);
PV_API pv_status_t pv_koala_batch_set_level_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const float *state /*[count][2]*/);
/* The same for the single-stream handle of pv_koala.h: the setting of pv_koala_process from the next frame on (pv_koala_reset makes its state fresh). */
PV_API pv_status_t pv_koala_set_level(pv_koala_t *object, const pv_koala_level_t *setting);
PV_API pv_status_t pv_koala_get_level(const pv_koala_t *object, pv_koala_level_t *setting);

/* COMFORT NOISE (twelfth extension): a low, stationary, spectrally shaped noise exactly where the mask removed energy,
 * so a hard-gated stream does not fall to digital silence between words -- and nothing on top of passed speech.  It is added in the spectrum
 * of the inner 16 kHz call, where the mask is applied: every rate, sample format, channel layout and packet handle gets it.  Per stream b
 * there is a SETTING (pv_koala_comfort_t: on, seed; a new handle: off), an AMPLITUDE CURVE A_b[k], k = 0 .. 256, fp32, finite and >= 0, in the
 * spectrum's units (the X of the FRAME REPORT: samples / 32768, sqrt-Hann, 512-point transform; koala_amd/comfort.py, curve(), turns an
 * output level in dBFS into A), and one uint32 of STATE, n_b: the number of frames the stream has completed since it was fresh, counted
 * only while its comfort noise is on, modulo 2^32.  In every frame a stream with comfort noise on completes, with m' the mask after the
 * attenuation limit and the band profile (exactly pv_koala_batch_set_band_profile's m'), n the counter's value and X the frame's spectrum:
 *     v  = seed ^ (n * 0x9E3779B9) ^ (k * 0x85EBCA6B)                          uint32, wrapping
 *     v ^= v >> 16;  v *= 0x7FEB352D;  v ^= v >> 15;  v *= 0x846CA68B;  v ^= v >> 16
 *     z_re = ((float) (v & 0xFFFF) - 32767.5f) * (1 / 32768)                   exact in fp32
 *     z_im = ((float) (v >> 16)    - 32767.5f) * (1 / 32768)                   0 for k = 0 and k = 256
 *     w = 1 - m'[k];  a = w * A[k];  Y_re = (m'[k] * X_re) + (a * z_re)        every operation rounded once, none fused; the same for im
 * the frame is synthesised from Y as it is from m' X otherwise, n becomes n + 1, and e_out of the frame report is that of Y (e_in and
 * mask_sum are unchanged).  So an fp32 handle stays bit-exact against the oracle under the rule (koala_amd/comfort.py states it in numpy).
 *   - min_gain = 1, or a band profile with floor = ceil = 1: m' = 1, w = 0 -- the handle is still the pure delay, bit for bit;
 *   - A = 0 delivers the samples of the stream with comfort noise off;
 *   - the network never sees its output: hidden state, history, stream records, e_in and mask_sum are bit for bit those of the handle
 *     without the feature;
 *   - configuration, not state: no reset, hold or record changes or carries the setting or the curve; records keep their version and bytes.
 *     The counter travels through pv_koala_batch_get_comfort_state / _set_comfort_state, four bytes for a caller that moves a stream;
 *   - pv_koala_batch_reset (all or masked), a per-frame `reset` at frame t and a packet call's `restart` make n = 0 before that frame; a
 *     held stream (`hold`, a stalled stream of a packet call) keeps n; a stream whose comfort noise is off does not count;
 *   - two streams with equal seed, curve, counter and input deliver equal samples; different seeds give different noise;
 *   - the output leveller runs behind the call and sees the samples with the noise in them;
 *   - host pointers on a plain 16 kHz handle: while some stream's comfort noise is on a call is one copy in, the device route, one copy out.
 * pv_koala_batch_set_comfort_noise: settings[i] (and amplitude[i], a row of 257; amplitude == NULL: every listed stream keeps its curve, all
 * zero on a new handle) belong to stream streams[i]; streams == NULL means slots 0 .. count - 1; streams not listed keep theirs.
 * `struct_size` of settings[0] is the distance between the entries: sizeof(pv_koala_comfort_t), or more from a later header.  All arrays
 * are HOST memory, read before the function returns.  Everything is checked before anything changes; PV_STATUS_INVALID_ARGUMENT with a
 * message that names the entry and the bin ("comfort 3, bin 17: ..."): an amplitude that is NaN, negative or infinite, `on` not 0 or 1, a bad
 * count, index, duplicate slot or struct_size.  No device work and no wait: the tables travel with the next call and are uploaded only
 * when they have changed.
 * pv_koala_batch_get_comfort_noise: the setting (the caller sets setting->struct_size) and the curve in force of one stream; either
 * out-pointer may be NULL.
 * pv_koala_batch_get_comfort_state / _set_comfort_state: n[i] = the counter of stream streams[i], HOST memory; they run on the handle's stream
 * behind everything enqueued and return when done (a handle that never filled answers 0 at once and allocates nothing).
 * NOT YET, refused by name with PV_STATUS_INVALID_ARGUMENT, nothing processed and state unchanged, while some stream's comfort noise is on:
 * a call with the channel link on, with the high-band carry on, through the asynchronous entry points, or on a handle at 44 100 / 22 050 Hz. */
typedef struct {
    int32_t struct_size; /* sizeof(pv_koala_comfort_t) */
    int32_t on;          /* 0: off (seed and curve are kept but unused), 1: on */
    uint32_t seed;       /* the stream's noise sequence */
} pv_koala_comfort_t;
PV_API pv_status_t pv_koala_batch_set_comfort_noise(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const pv_koala_comfort_t *settings,
                                                    const float *amplitude /*[count][257] or NULL: keep*/);
PV_API pv_status_t pv_koala_batch_get_comfort_noise(const pv_koala_batch_t *object, int32_t stream, pv_koala_comfort_t *setting /*or NULL*/,
                                                    float *amplitude /*[257] or NULL*/);
PV_API pv_status_t pv_koala_batch_get_comfort_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, uint32_t *n /*[count]*/);
PV_API pv_status_t pv_koala_batch_set_comfort_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const uint32_t *n /*[count]*/);
/* The same for the single-stream handle of pv_koala.h: the setting of pv_koala_process from the next frame on (pv_koala_reset makes n = 0). */
PV_API pv_status_t pv_koala_set_comfort_noise(pv_koala_t *object, const pv_koala_comfort_t *setting, const float *amplitude /*[257] or NULL: keep*/);
PV_API pv_status_t pv_koala_get_comfort_noise(const pv_koala_t *object, pv_koala_comfort_t *setting /*or NULL*/, float *amplitude /*[257] or NULL*/);

/* PEAK LIMITER (thirteenth extension): a per-stream ceiling on the output with instant attack and linear release -- what
 * stands behind the output leveller, and what a caller who must stay under -1 dBFS in front of a codec, or -3 dBFS in front of a G.711
 * trunk, turns on.  It works on the samples E of the inner 16 kHz call, on the device, in the leveller's place and in one launch with its
 * ramp (it sees the product before saturation): every rate, sample format, channel layout and packet handle gets it.  Per stream b there
 * is a SETTING (pv_koala_limiter_t; a new handle: off) -- `ceiling` c in sample units, 1 <= c <= 32767, and `release` delta, the gain
 * recovered per 16 kHz sample, 0 < delta <= 1 -- and one fp32 value of STATE, g, the gain behind the stream's last sample; fresh: g = 1.
 * For every frame t that a stream with the limiter on completes in a call that does not hold it, n = 0 .. 255, all in fp32, one rounding
 * per operation, none contracted, in this order:
 *     r[n]   = fmaf(n / 256, g_t - g_{t-1}, g_{t-1})     if the stream's leveller is on (the tracker's pair of this frame), else 1
 *     v[n]   = float(E[256 t + n]) * r[n]                 -- the leveller's own product, BEFORE to_pcm
 *     q[n]   = 1 if |v[n]| <= c else c / |v[n]|           -- the correctly rounded division
 *     m_0    = q
 *     m_{j+1}[n] = min(m_j[n], m_j[n - 2^j] + (2^j delta))   for n >= 2^j, else m_j[n]        j = 0 .. 7   (2^j delta is exact)
 *     h[n]   = fmaf(float(n + 1), delta, g)               -- g: the state entering this frame
 *     G[n]   = min(1, min(m_8[n], h[n]))
 *     out[256 t + n] = to_pcm(v[n] * G[n]);   g := G[255]
 * to_pcm is the leveller's.  m_8 is the lower envelope min_k (q[n - k] + k delta) inside the frame and h carries the release over the frame
 * boundary: the gain falls to q at once and recovers by delta per sample, within 9 * 2^-23 of the per-sample recursion
 * min(1, q[n], g[n - 1] + delta), and exactly the same however the frames are cut into calls.  G <= q, so for an integer c no output
 * sample of a limiting stream is above c in magnitude; where G is 1 throughout, the output is the leveller's (or E) bit for bit.
 * THE CEILING IS A STATEMENT ABOUT THE INNER 16 kHz SAMPLES: the interpolator of an out-stage (a handle at another rate) or a G.711
 * encoder behind it can overshoot it by a little -- leave that margin in c.  koala_amd/limiter.py, settings(), turns dBFS and milliseconds
 * into the fields, and states the rule in numpy.
 *   - a per-frame `reset` at frame t, a packet call's `restart` and pv_koala_batch_reset (masked or not) set g = 1 before that frame;
 *   - a held stream (`hold`, a stalled stream of a packet call) keeps g, and its samples are not touched;
 *   - a stream whose limiter is off delivers what it delivered before and its g does not move; a handle on which no stream limits runs the
 *     launches, and delivers the bits, it always did;
 *   - the frame report is untouched: column 3 stays the leveller's gain, and e_out stays in front of both;
 *   - the setting is configuration: no reset, hold or record changes or carries it.  Stream records do not change; the float travels
 *     through pv_koala_batch_get_limiter_state / _set_limiter_state, four more bytes for a caller that moves a stream;
 *   - host pointers on a plain 16 kHz handle, the single-stream handle included: while some stream limits a call is one copy in, the
 *     device route, one copy out.
 * pv_koala_batch_set_limiter / _get_limiter / _get_limiter_state / _set_limiter_state: every convention (`struct_size` as the distance
 * between entries, streams == NULL, host memory, index checks, everything checked before anything changes) is pv_koala_batch_set_level's;
 * state[i] is g of stream streams[i]; g not in (0, 1], NaN or infinity is refused; a handle that never limited answers 1 at once.
 * NOT YET, refused by name with PV_STATUS_INVALID_ARGUMENT, nothing processed and state unchanged, while some stream's limiter is on: a
 * call with the channel link on (a stereo limiter must be linked), with the high-band carry on, through the asynchronous entry points, or
 * on a handle at 44 100 / 22 050 Hz. */
typedef struct {
    int32_t struct_size; /* sizeof(pv_koala_limiter_t) */
    int32_t on;          /* 0: off (the other fields are kept but unused), 1: on */
    float ceiling;       /* c, in sample units, in [1, 32767] */
    float release;       /* delta, the gain recovered per 16 kHz sample, in (0, 1] */
} pv_koala_limiter_t;
PV_API pv_status_t pv_koala_batch_set_limiter(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const pv_koala_limiter_t *settings);
PV_API pv_status_t pv_koala_batch_get_limiter(const pv_koala_batch_t *object, int32_t stream, pv_koala_limiter_t *setting);
PV_API pv_status_t pv_koala_batch_get_limiter_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, float *state /*[count]*/);
PV_API pv_status_t pv_koala_batch_set_limiter_state(pv_koala_batch_t *object, int32_t count, const int32_t *streams, const float *state /*[count]*/);
/* The same for the single-stream handle of pv_koala.h: the setting of pv_koala_process from the next frame on (pv_koala_reset sets g = 1). */
PV_API pv_status_t pv_koala_set_limiter(pv_koala_t *object, const pv_koala_limiter_t *setting);
PV_API pv_status_t pv_koala_get_limiter(const pv_koala_t *object, pv_koala_limiter_t *setting);

PV_API pv_status_t pv_koala_batch_num_streams(const pv_koala_batch_t *object, int32_t *num_streams);
PV_API pv_status_t pv_koala_batch_delay_sample(const pv_koala_batch_t *object, int32_t *delay_sample);

/* Page-locked host memory for `pcm` / `enhanced`.  Host-pointer calls are pipelined in sub-chunks (copy-in, kernels and
 * copy-out of consecutive sub-chunks overlap); buffers obtained here -- or any other page-locked memory -- are read and
 * written by the GPU's copy engines directly, ordinary (pageable) buffers go through the handle's staging slots first.
 * Not tied to a handle; release with pv_koala_batch_host_free (NULL is accepted). */
PV_API pv_status_t pv_koala_batch_host_alloc(int64_t num_bytes, void **memory);
PV_API void pv_koala_batch_host_free(void *memory);

/* Run on a caller-provided HIP stream (a hipStream_t passed as void*; NULL = the handle's own stream).  Changing the stream first
 * waits for everything the handle has in flight (asynchronous host calls, work queued on the previous stream -- which must still
 * exist), since the next call's kernels work on the same stream state. */
PV_API pv_status_t pv_koala_batch_set_stream(pv_koala_batch_t *object, void *hip_stream);
/* Blocks until everything enqueued by this handle -- device-pointer calls, asynchronous host calls -- has finished. */
PV_API pv_status_t pv_koala_batch_synchronize(pv_koala_batch_t *object);

/* Per-kernel timing with HIP events recorded on the handle's stream (bench.py's roofline leg).
 * kernel classes: 0 analysis, 1 input-side GEMMs, 2 recurrent GRU, 3 head/front-end GEMMs, 4 synthesis. */
#define PV_KOALA_NUM_KERNEL_CLASSES 5
PV_API pv_status_t pv_koala_batch_profile_enable(pv_koala_batch_t *object, int32_t enable);
PV_API pv_status_t pv_koala_batch_profile_read(pv_koala_batch_t *object, double *milliseconds /*[5]*/,
                                               int64_t *launches /*[5]*/);

/* Debug taps of the last processed chunk, copied to host in logical (unpacked) layout; used by the parity tests.
 * what: 0 features [T][B][257], 1 spectrum [T][B][257][2], 2 mask [T][B][257], 3 hidden state [8][B][271],
 *       4 embedding e [T][B][271].  Returns the number of floats written, or a negative pv_status_t. */
PV_API int64_t pv_koala_batch_debug_read(pv_koala_batch_t *object, int32_t what, float *out, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* PV_KOALA_BATCH_H */
