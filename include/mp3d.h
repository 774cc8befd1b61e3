/*
 * mp3d.h -- C ABI of the MI355X-native batched MP3 (MPEG-1 and MPEG-2 / 2.5
 * Layer III) decoder.
 *
 * Drop-in boundary for the decode hot path of lxm0851/mp3.  The reference
 * snapshot contains no decoder source and therefore no FFI surface to copy
 * (SURVEY.md §8(b)): the player it describes (REF/README.md:2-3, "audio
 * player ... crackle and noise during playback") decodes MP3 frame by frame
 * in its playback loop, and REF/README.md:44 says it runs from source.  The
 * per-frame entry point below replaces that (absent) per-frame decode call
 * with the conventional shape of public C MP3 decoders (decoder handle,
 * frame bytes in, interleaved int16 PCM + frame info out); the batch entry
 * points expose the same path for tens of thousands of concurrent streams.
 * INTEGRATION.md shows the ctypes / cffi / C++ bindings a host adds.
 *
 * Conventions
 *  - Plain C types only.  All calls return >= 0 on success, a negative
 *    MP3D_E* code on failure; nothing throws or aborts across the ABI.
 *  - Caller owns every buffer passed in.  A handle owns its device memory
 *    and decoder state; *_destroy frees it.
 *  - PCM is int16 (or float32 with the _f32 entry points), interleaved L/R,
 *    1152 samples per channel per MPEG-1 frame, 576 per MPEG-2 / 2.5 (LSF)
 *    frame, at the start of the frame's 2304-sample row.
 *  - The compute path is HIP on an AMD Instinct MI355X (gfx950).  There is
 *    no CPU fallback: without a usable GPU, create calls fail with
 *    MP3D_E_NO_DEVICE.
 */
#ifndef MP3D_H
#define MP3D_H

#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5: the state blob's synthesis history is partial window sums in float
 *    units, with a format stamp (blobs of v4 are refused by set_state) */
#define MP3D_ABI_VERSION 5

#if defined(__GNUC__) || defined(__clang__)
#define MP3D_API __attribute__((visibility("default")))
#else
#define MP3D_API
#endif

/* error codes */
#define MP3D_OK 0
#define MP3D_E_ARG (-1)        /* bad argument                                 */
#define MP3D_E_NO_DEVICE (-2)  /* no HIP device / device ordinal out of range  */
#define MP3D_E_HIP (-3)        /* HIP runtime error (see mp3d_last_hip_error)  */
#define MP3D_E_NOMEM (-4)      /* device or host allocation failed             */
#define MP3D_E_CAPACITY (-5)   /* batch larger than the handle was created for */
#define MP3D_E_NEED_MORE (-6)  /* buffer holds no complete frame               */

typedef struct mp3d_frame_info {
    int frame_bytes;  /* bytes consumed (0: no frame found)                */
    int channels;     /* 1 or 2                                            */
    int hz;           /* 32000 / 44100 / 48000 (MPEG-1), 8000 .. 24000 LSF */
    int layer;        /* 3                                                 */
    int bitrate_kbps; /* 32..320 (MPEG-1), 8..160 (LSF)                    */
    int samples;      /* PCM samples per channel: 1152, 576 (LSF) or 0    */
} mp3d_frame_info;

typedef struct mp3d_dec mp3d_dec;
typedef struct mp3d_batch mp3d_batch;

/* ---- per-frame decoder (the player's decode call) ---------------------- *
 * One decoder per audio stream and host thread.  mp3d_decode_frame finds
 * the next frame in buf (skipping an ID3v2 tag / garbage before the sync
 * word), decodes it on the GPU and returns samples per channel: 1152 (576
 * for an MPEG-2 / 2.5 LSF frame), or 0
 * when bytes were consumed without audio (Xing/Info tag frame, invalid
 * frame).  info->frame_bytes (+ any skipped prefix) tells how far to
 * advance; pcm may be NULL (decode for state only).  Reservoir underflow
 * (a stream entered mid-way) follows FFmpeg: the affected granules decode
 * as silence.  A HIP error while the decoder was reading ahead (or putting
 * a read-ahead back) leaves its state undefined: that error is returned by
 * every later decode / get_state / set_options call until mp3d_dec_reset or
 * a successful mp3d_dec_set_state.                                          */
MP3D_API int mp3d_dec_create(mp3d_dec **out);
MP3D_API int mp3d_dec_create_on(int device, mp3d_dec **out);
MP3D_API void mp3d_dec_destroy(mp3d_dec *dec);
MP3D_API void mp3d_dec_reset(mp3d_dec *dec);
MP3D_API int mp3d_decode_frame(mp3d_dec *dec, const uint8_t *buf, size_t bytes, int16_t *pcm /* <= 2304 */,
                      mp3d_frame_info *info);
/* the same with float32 PCM (FFmpeg's float convention: full scale 1.0,
 * not clipped; the int16 output is clamp(floor(x * 32768 + 0.5)) of these
 * values, saturated to [-32768, 32767]: FFmpeg's fixed-point round_sample
 * convention, so an exact .5 tie rounds up, unlike rint's ties-to-even) */
MP3D_API int mp3d_decode_frame_f32(mp3d_dec *dec, const uint8_t *buf, size_t bytes, float *pcm /* <= 2304 */,
                          mp3d_frame_info *info);
/* (ABI v4) either of the above by flags: MP3D_FRAME_F32 selects float32 PCM;
 * MP3D_FRAME_LAST says buf holds the rest of the stream, so a final frame cut
 * short (header and side info present) is decoded with its missing bytes as
 * zeros -- as the batch path and FFmpeg do -- instead of MP3D_E_NEED_MORE;
 * info->frame_bytes then counts the bytes that were present.              */
#define MP3D_FRAME_F32 1
#define MP3D_FRAME_LAST 2
MP3D_API int mp3d_decode_frame_ex(mp3d_dec *dec, const uint8_t *buf, size_t bytes, void *pcm, int flags,
                                  mp3d_frame_info *info);

/* ---- batched decoder (many concurrent streams on one GPU) -------------- *
 * A batch handle keeps per-stream decoder state resident in HBM across
 * calls: call k decodes frames [k*F, (k+1)*F) of every stream.
 *
 * frames           all streams' bytes; host memory or a device pointer on
 *                  the handle's GPU (detected per call)
 * offsets, sizes   host arrays [n_streams]: stream s occupies
 *                  frames[offsets[s] .. offsets[s] + sizes[s])
 * pcm              [n_streams][frames_per_stream][2304] int16, host or
 *                  device; frames with info.samples == 0 are left untouched
 * infos            [n_streams][frames_per_stream] or NULL, host or device
 * hip_stream       hipStream_t to run on (NULL: the handle's own stream)
 * The call is asynchronous when every pointer is device memory; otherwise
 * it synchronises before returning.                                         */
MP3D_API int mp3d_batch_create(int device, int max_streams, int max_frames, mp3d_batch **out);
MP3D_API void mp3d_batch_destroy(mp3d_batch *b);
MP3D_API int mp3d_batch_reset(mp3d_batch *b); /* forget all per-stream state         */
MP3D_API int mp3d_batch_decode(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets, const uint32_t *sizes,
                      int n_streams, int frames_per_stream, int16_t *pcm, mp3d_frame_info *infos,
                      void *hip_stream);
/* float32 PCM sink: pcm [n_streams][frames_per_stream][2304] float */
MP3D_API int mp3d_batch_decode_f32(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                          const uint32_t *sizes, int n_streams, int frames_per_stream, float *pcm,
                          mp3d_frame_info *infos, void *hip_stream);
MP3D_API int mp3d_batch_sync(mp3d_batch *b);

/* ---- decode options (ABI v3) --------------------------------------------- *
 * MP3D_OPT_CRC_CHECK: verify the CRC-16 of error-protected frames (ISO
 *   11172-3 2.4.3.1: polynomial 0x8005 over header bytes 2..3 and the side
 *   info) and drop a frame whose CRC mismatches, like a bad frame
 *   (info.samples = 0; the bit reservoir restarts from the frame's own
 *   bytes).  FFmpeg behaves so with err_detect = crccheck + explode; its
 *   default, and this library's, ignores the CRC.
 * Options apply to later decode calls of the handle.                        */
#define MP3D_OPT_CRC_CHECK 1
MP3D_API int mp3d_batch_set_options(mp3d_batch *b, int flags);
MP3D_API int mp3d_dec_set_options(mp3d_dec *dec, int flags);

/* ---- staged entry points (parity taps / BASELINE config 2) ------------- *
 * huffman_only: run demux + reservoir + scalefactors + Huffman and return
 *   is_out [n_streams][F][2][2][576] int16 and sf_out [..][2][2][40] uint8
 *   (either may be NULL).  Advances per-stream state like a decode.
 * synth_only: stages a8..a11 from spectra: xr [n_streams][F][2 gr][nch][576]
 *   f32 (requantised, after stereo, bitstream order), block_type / mixed
 *   [n_streams][F][2][nch]; pcm as in mp3d_batch_decode.                    */
MP3D_API int mp3d_batch_huffman_only(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets, const uint32_t *sizes,
                            int n_streams, int frames_per_stream, int16_t *is_out, uint8_t *sf_out,
                            void *hip_stream);
/* synth_only takes MPEG-1 rates (32 / 44.1 / 48 kHz) */
MP3D_API int mp3d_batch_synth_only(mp3d_batch *b, const float *xr, const uint8_t *block_type, const uint8_t *mixed,
                          int n_streams, int frames_per_stream, int nch, int sample_rate_hz, int16_t *pcm,
                          void *hip_stream);

/* ---- stream-level info: Xing/Info tag and gapless playback ------------- *
 * Filled from the stream's leading Xing/Info frame (read by the demux kernel
 * on the stream's first call).  Gapless trim follows FFmpeg's demuxer
 * (libavformat/mp3dec.c): with a LAME / Lavf / Lavc encoder extension the
 * first enc_delay + 529 decoded samples per channel are encoder/decoder
 * delay, and when the tag also carries a frame count, samples from
 * total_frames * 1152 (576 for MPEG-2/2.5 LSF) + 529 - enc_padding on are padding.  The decoder
 * always emits every decoded frame; apply the trim when concatenating.      */
typedef struct mp3d_stream_info {
    int has_tag;          /* a Xing/Info frame opened the stream               */
    int has_lame;         /* ... with a LAME / Lavf / Lavc encoder extension   */
    int enc_delay;        /* encoder delay, samples per channel (0 if none)    */
    int enc_padding;      /* encoder padding, samples per channel (0 if none)  */
    int total_frames;     /* Xing frame count (-1 if absent)                   */
    int skip_samples;     /* gapless: leading samples to drop (0 if none)      */
    long long end_sample; /* gapless: index of the first padding sample, -1    */
} mp3d_stream_info;

/* out[n_streams]; valid once the call that decoded a stream's first frame
 * has completed (synchronises the handle's stream).                       */
MP3D_API int mp3d_batch_stream_info(mp3d_batch *b, int n_streams, mp3d_stream_info *out);
MP3D_API int mp3d_dec_stream_info(mp3d_dec *dec, mp3d_stream_info *out);

/* ---- one long stream at full-GPU speed (frame-parallel) ---------------- *
 * Decodes a whole stream (data[0 .. bytes), host or device) by splitting it
 * into segments of L output frames that run as concurrent virtual streams
 * of one batch call.  Each segment starts a few frames early (payloads of
 * >= 511 bytes, the largest main_data_begin, before its first frame but one),
 * so its output is bit-identical to a sequential decode; the warm-up frames'
 * output is discarded.  The handle (mp3d_batch_create) needs max_streams
 * >= 1 and max_frames >= L + 11: the warm-up is 4 frames at 128 kbps
 * stereo and at most 11 (32 kbps); more max_streams runs more segments per
 * kernel launch.
 * pcm     [max_frames][2304] int16, or float with f32 != 0; host or device.
 *         Row j is frame slot j of the stream, zero for slots without
 *         audio (Xing/Info frame, dropped frame); a mono row holds 1152
 *         samples and zeros.
 * infos   [max_frames] or NULL, host or device.
 * n_frames   out: frame slots found (MP3D_E_CAPACITY if > max_frames).
 * sinfo   stream info (Xing/Info tag, gapless trim) or NULL.
 * Synchronous.  The segments decode on scratch state: the handle's own
 * per-stream state (for mp3d_batch_decode) is left untouched.              */
MP3D_API int mp3d_batch_decode_long(mp3d_batch *b, const uint8_t *data, size_t bytes, int L, void *pcm, int f32,
                                    long long max_frames, mp3d_frame_info *infos, long long *n_frames,
                                    mp3d_stream_info *sinfo);

/* Host-side plan of mp3d_batch_decode_long (no GPU needed): the stream's
 * frame slots (frame_off[n_frames], byte offset of each frame header) and
 * the first frame of each segment's warm-up (seg_start[ceil(n_frames / L)]);
 * either array may be NULL.  max_warmup = max over segments of
 * k * L - seg_start[k].  data must be host memory.  A caller can shard the
 * segments of one stream over several GPUs with it.                        */
MP3D_API int mp3d_long_plan(const uint8_t *data, size_t bytes, int L, long long max_frames, uint64_t *frame_off,
                            long long *seg_start, long long *n_frames, int *max_warmup);

/* ---- per-stream state save / restore (ABI v4) --------------------------- *
 * A stream's decoder state -- bit-reservoir carry, IMDCT overlap, synthesis
 * history, MPEG family, Xing/LAME tag, frame count -- is an opaque blob of
 * mp3d_state_bytes() bytes, valid for handles of the same ABI version and
 * for either PCM sink (a stream may switch between int16 and float calls).
 * batch_get_state copies the state of streams [first, first + n) out of the
 * handle into buf; batch_set_state writes it into those slots (of this or
 * another handle) and fails with MP3D_E_ARG, writing nothing, when a blob
 * lacks this version's format stamp (e.g. one saved by an ABI v4 build).  A player seeks by saving the state at a frame boundary
 * and restoring it before decoding from that frame's bytes again; a server
 * moves a stream between batches or GPUs the same way.  buf: host or device
 * memory.  Both order after the handle's last call and return when done.  */
MP3D_API size_t mp3d_state_bytes(void);
MP3D_API int mp3d_batch_get_state(mp3d_batch *b, int first, int n, void *buf);
MP3D_API int mp3d_batch_set_state(mp3d_batch *b, int first, int n, const void *buf);
MP3D_API int mp3d_dec_get_state(mp3d_dec *dec, void *buf);
MP3D_API int mp3d_dec_set_state(mp3d_dec *dec, const void *buf);

/* ---- packed uniform-rate PCM sink --------------------------------------- *
 * Instead of [n][F][2304] rows at each stream's own rate and channel count,
 * a packed call writes every stream's samples contiguously at ONE rate and
 * channel count, resampled and down/up-mixed on the GPU.  The resampler keeps
 * per-stream state in the handle (not in the state blob), so a stream decoded
 * in calls of any size gives the same samples as one call.
 *
 * Filter (for in_hz, out_hz from 8000, 11025, 12000, 16000, 22050, 24000,
 * 32000, 44100, 48000):
 *   g = gcd(in_hz, out_hz); L = out_hz / g; M = in_hz / g
 *   r = min(1, L / M); W = 24 / r; T = 2 ceil(W)        taps per phase
 *   t = p / L - (j - (T/2 - 1))
 *   w = I0(9 sqrt(1 - (t/W)^2)) / I0(9) for |t| < W, else 0   (Kaiser, beta 9)
 *   h = 0.88 r sinc(0.88 r t) w;   taps[p][j] = h / sum_j h
 *   y[m] = sum_j taps[p][j] x[n0 - (T/2 - 1) + j], n0 = floor(m M / L),
 *   p = (m M) mod L, x[n < 0] = 0: y[m] sits at time m / out_hz, no delay.
 * The products are accumulated in float32 in ascending j.  in_hz == out_hz
 * is a bypass (L = M = T = 1): the samples are copied.  Before the filter
 * the channels are mapped: mono -> stereo duplicates, stereo -> mono is
 * 0.5f * (l + r); a stream may switch between mono and stereo frames.
 *
 * A stream's input rate is fixed by its first audio frame after a restart;
 * later frames that report another hz are fed at that rate (their infos keep
 * their own hz).  An output is emitted once every input it needs has been
 * seen (n0 + T/2 <= inputs seen - 1); the tail waits for the next call.  A
 * stream's resampler restarts (history zero, m = 0) at create, at
 * mp3d_batch_reset, at mp3d_batch_set_state on its slot, at a change of the
 * output format, and after its own flush.
 *
 * Sample windows.  Each stream slot of a handle with a packed format set has
 * a fed count r and a window [lo, hi), both in input samples per channel at
 * the stream's own rate.  r counts the samples of the audio frame slots the
 * sink has been fed (0 < samples <= 1152, 1 or 2 channels, after the rate is
 * known).  Input sample number r of the slot reaches the channel map and the
 * resampler only if lo <= r < hi; the resampler sees the kept samples as one
 * contiguous signal, and its time axis, history, emit rule and flush rule
 * are the ones above with "inputs seen" meaning kept inputs.  r advances by
 * every sample fed, kept or not, written or not (a stride overflow,
 * out_count = -1, still advances it).  The input rate is still fixed by the
 * first audio frame after a resampler restart, kept or trimmed.
 *
 * A window restart sets r = 0 and the window to "not fixed".  It happens
 * where the resampler state is zeroed (create, mp3d_batch_reset,
 * mp3d_batch_set_state on the slot, mp3d_batch_set_output) and at
 * mp3d_batch_set_window on the slot.  MP3D_PACK_FLUSH, a stride overflow and
 * mp3d_batch_set_features are NOT window restarts: they restart the
 * resampler and the feature state, r and the window carry on (a flush is not
 * a stream start: a stream flushed mid-file and continued does not have its
 * head trimmed a second time).
 *
 * mp3d_batch_set_window fixes the window at once, and MP3D_PACK_GAPLESS is
 * then ignored.  Otherwise the window is fixed by the first packed or feature
 * call after the restart that feeds the slot at least one sample: if that
 * call carries MP3D_PACK_GAPLESS and the stream's Xing/Info tag has a LAME /
 * Lavf / Lavc extension, lo = enc_delay + 529 (skip_samples) and hi =
 * total_frames * spf + 529 - enc_padding (end_sample) when the tag carries a
 * frame count > 0 and that end is >= 0, else no end: mp3d_stream_info's
 * values and mp3d_batch_decode_long_packed's trim.  Without the flag or such
 * a tag the window is [0, no end).  Once fixed, the flag of later calls is
 * ignored for the slot until its next window restart.  With no flag and no
 * explicit window every call produces exactly the bits it produced without
 * windows.  A window only removes samples, so mp3d_packed_max_samples and
 * mp3d_feat_max_frames stay valid bounds.
 *
 * mp3d_batch_set_state leaves the window unfixed with r = 0, so a state
 * restored mid-file counts from the restore point; a caller moving a stream
 * mid-file reads its window with mp3d_batch_sink_window and sets
 * (max(lo - r, 0), max(hi - r, 0)) (no end stays no end) on the destination. */

/* host only, no GPU: taps[L][T] floats (NULL: sizes only); cap = floats taps
 * can hold; returns L * T or MP3D_E_ARG */
MP3D_API long long mp3d_resample_filter(int in_hz, int out_hz, int *L, int *M, int *T, float *taps, size_t cap);

/* out_hz from the nine rates, out_channels 1 or 2; out_hz = 0 turns the sink
 * off and frees its buffers.  Waits for the handle's work. */
MP3D_API int mp3d_batch_set_output(mp3d_batch *b, int out_hz, int out_channels);

/* smallest out_stride that can never overflow: the most samples per channel
 * one call of `frames` frames per stream can emit for any input rate
 * >= min_in_hz (the pending tail of earlier calls included); 0 when
 * min_in_hz is above 48000 */
MP3D_API long long mp3d_packed_max_samples(int out_hz, int frames, int min_in_hz);

/* Decodes like mp3d_batch_decode_f32 (the decoder state advances exactly so),
 * then stream s writes out_count[s] samples per channel, interleaved, at
 * out + s * out_stride * out_channels elements; nothing past them is touched.
 * out is float32 when f32 != 0, else int16 (clamp(floor(y * 32768 + 0.5))).
 * out, out_count and infos (may be NULL) are host or device memory; the call
 * is asynchronous when all of them are device memory.  MP3D_PACK_FLUSH feeds
 * zeros after the call's frames, so a stream's lifetime total is exactly
 * ceil(N L / M) for its N input samples, and its resampler restarts.  A
 * stream that would exceed out_stride gets out_count[s] = -1, writes nothing
 * and has its resampler restarted.  MP3D_E_ARG before mp3d_batch_set_output.
 * A device out must be aligned to one sample frame (out_channels elements: 8
 * bytes for float32 stereo, 4 for int16 stereo or float32 mono), else
 * MP3D_E_ARG; a host out may sit anywhere.  A host (or other-GPU) out is
 * filled from a staging buffer by one copy of out_count[s] samples per
 * stream, which keeps the bytes past them untouched but costs n_streams
 * copies per call: meant for small batches, wide ones pass device memory.
 * flags: MP3D_PACK_FLUSH, MP3D_PACK_GAPLESS (sample windows, above); any
 * other bit is MP3D_E_ARG.                                                  */
#define MP3D_PACK_FLUSH 1
#define MP3D_PACK_GAPLESS 2
MP3D_API int mp3d_batch_decode_packed(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                      const uint32_t *sizes, int n_streams, int frames_per_stream, void *out, int f32,
                                      long long out_stride, int *out_count, int flags, mp3d_frame_info *infos,
                                      void *hip_stream);

/* Fixes the sample windows [lo[i], hi[i]) of slots [first, first + n) (host
 * arrays of n; hi == NULL: no end for all; an element MP3D_WINDOW_NO_END: no
 * end for that slot).  lo == NULL && hi == NULL un-fixes them, a plain window
 * restart.  Either way the slots' resampler state, fed count and (when
 * features or loudness are set) feature and loudness state restart first.  Orders after the handle's
 * last call and returns when done.  MP3D_E_ARG, writing nothing: no packed
 * format set, lo[i] < 0, hi[i] < lo[i], or hi without lo.  MP3D_E_CAPACITY:
 * the range is past max_streams.                                            */
#define MP3D_WINDOW_NO_END LLONG_MAX
MP3D_API int mp3d_batch_set_window(mp3d_batch *b, int first, int n, const long long *lo, const long long *hi);

/* The slots' windows and fed counts r into host arrays of n; any of the three
 * may be NULL.  A slot whose window is not fixed reports 0,
 * MP3D_WINDOW_NO_END, 0.  Orders after the handle's last call and returns
 * when done, as mp3d_batch_get_state does; errors as above.                 */
MP3D_API int mp3d_batch_sink_window(mp3d_batch *b, int first, int n, long long *lo, long long *hi, long long *fed);

/* device-side microseconds of the resample stage of the last packed call, or
 * of the last chunk of the last mp3d_batch_decode_long_packed call (a stream
 * of up to max_streams segments is one chunk); needs mp3d_batch_set_timing */
MP3D_API int mp3d_batch_resample_time(mp3d_batch *b, float *us);

/* ---- one long stream into the packed format (a player's open-file path) -- *
 * Decodes a whole stream exactly as mp3d_batch_decode_long does (same L, same
 * warm-up, max_frames >= L + 11, on scratch state) and writes it as ONE run
 * of interleaved samples at out_hz and out_channels, gapless: the segments'
 * rows are channel-mapped, trimmed and resampled on the GPU chunk by chunk,
 * without an intermediate [n_frames][2304] buffer.
 *
 * Input signal x: the stream's frame slots in order; a slot with samples > 0
 * contributes its samples per channel, a slot without audio (Xing/Info
 * frame, dropped frame, garbage) nothing.  The input rate is fixed by the
 * first audio frame, as in the packed sink; later frames that report another
 * hz are fed at that rate.  *in_hz (may be NULL) gets it, 0 without audio.
 * The channel map is the packed sink's, per frame, before the filter, in
 * float32: mono -> stereo duplicates, stereo -> mono is 0.5f * (l + r).
 *
 * Trim: with MP3D_LONG_GAPLESS and a LAME / Lavf / Lavc extension in the
 * stream's Xing/Info tag, x becomes x[skip_samples : stop], stop =
 * min(end_sample, N) when end_sample >= 0, else N (mp3d_stream_info; FFmpeg
 * semantics), in the input domain, before resampling.  Without the flag or
 * such a tag x is untouched.  The resampler sees the trimmed signal starting
 * at time 0 with zero history.
 *
 * Output: the packed sink's filter, flushed: exactly ceil(N' L / M) samples
 * per channel for the N' inputs left after the trim,
 *   y[m] = sum_j taps[p][j] x[n0 - (T/2 - 1) + j],  x outside [0, N') = 0,
 * each accumulated by one float32 FMA chain in ascending j whatever block,
 * tile or chunk computes it, so the samples are bit-identical to a flushed
 * mp3d_batch_decode_packed of the same stream, for any L and max_streams.
 * Equal rates are a copy.  f32 != 0: float32, else int16
 * (clamp(floor(y * 32768 + 0.5))).  Samples are interleaved and contiguous
 * from out.
 *
 * out is host or device memory of out_cap samples per channel; a device out
 * must be aligned to one sample frame, else MP3D_E_ARG.  Nothing at or past
 * out + out_cap * out_channels is touched, and nothing past the samples
 * written.  *out_samples is always the full count; when it exceeds out_cap
 * the first out_cap samples are written and valid and the call returns
 * MP3D_E_CAPACITY.  sinfo (may be NULL) gets the stream info.
 *
 * Synchronous.  Needs no mp3d_batch_set_output and leaves the handle's
 * output format, its resampler states, its per-stream decoder state and its
 * options as they were.  MP3D_E_ARG: out_hz not one of the nine rates,
 * out_channels not 1 or 2, NULL out_samples, L <= 0.                        */
#define MP3D_LONG_GAPLESS 1
MP3D_API int mp3d_batch_decode_long_packed(mp3d_batch *b, const uint8_t *data, size_t bytes, int L, int out_hz,
                                           int out_channels, void *out, int f32, long long out_cap,
                                           long long *out_samples, int flags, mp3d_stream_info *sinfo, int *in_hz);

/* host only, no GPU: walks the frames as mp3d_long_plan does and returns
 * ceil(n_slots * spf * L / M), spf (1152, LSF 576) and the input rate from
 * the first slot's header: an upper bound of *out_samples for any flags.
 * MP3D_E_ARG for a bad rate or a device pointer. */
MP3D_API long long mp3d_long_packed_bound(const uint8_t *data, size_t bytes, int out_hz);

/* ---- log-mel feature sink (a recogniser's front end) --------------------- *
 * Input signal of a stream: its packed-sink output at 16 000 Hz, 1 channel,
 * float32: x[0 .. N) since the stream's last restart.
 *
 * Frame t is centred on sample 160 t and covers x[160 t - 200 .. 160 t + 200),
 * with x outside [0, N) = 0 (25 ms frames every 10 ms).
 *   w[n] = 0.5 - 0.5 cos(2 pi n / 400), n = 0 .. 399          (periodic Hann)
 *   X[k] = sum_n w[n] x[160 t - 200 + n] exp(-2 pi i n k / 400), k = 0 .. 200
 *   P[k] = Re^2 + Im^2
 * Mel scale, Slaney form (linear up to 1 kHz, then logarithmic):
 *   mel(f) = 3 f / 200 for f < 1000, else 15 + ln(f / 1000) 27 / ln 6.4;
 *   hz(m) is its inverse
 *   c_i = hz(i mel(8000) / (n_mels + 1)), i = 0 .. n_mels + 1;  f_k = 40 k
 *   F[j][k] = max(0, min((f_k - c_j) / (c_j+1 - c_j),
 *                        (c_j+2 - f_k) / (c_j+2 - c_j+1))) 2 / (c_j+2 - c_j)
 * computed in double and rounded to float; 1 <= n_mels <= 128.
 *   mel[t][j] = sum_k F[j][k] P[k]
 * Output feat[s][t][j], float32, time-major: mel[t][j], or with
 * MP3D_FEAT_LOG10 log10(max(mel[t][j], 1e-10)).  There is no per-clip
 * normalisation: a clip maximum is the caller's.
 *
 * Emit rule: frame t is emitted once sample 160 t + 199 has been seen, so
 * after N samples a stream has emitted E(N) = floor((N - 200) / 160) + 1
 * frames for N >= 200, else 0.  MP3D_PACK_FLUSH also emits every frame with
 * 160 t < N, with zeros past N: the lifetime total is exactly ceil(N / 160),
 * and the stream's feature state restarts.
 *
 * A frame's values are the same bits whatever call, tile or position in a
 * tile computes it: every frame runs one fixed sequence of float32
 * operations (a 200-point complex FFT of the packed real frame, the
 * real-input unpack, the power, and each filter's products accumulated by
 * one FMA chain in ascending k).  Against the exact value, with
 * A = sum_n |w[n] x[n]| over the frame and d = 408 * 2^-24 * A,
 *   |mel - exact| <= (sum_k F[j][k]) (2 sqrt 2 A d + 2 d^2) + 8 * 2^-24 exact.
 *
 * The per-stream feature state (a sample count and a carry of at most 399
 * samples) lives in the handle while features are set, not in the state
 * blob.  It restarts where the resampler's does: at create, at
 * mp3d_batch_reset, at mp3d_batch_set_state on its slot, at
 * mp3d_batch_set_output (which also turns features off), at
 * mp3d_batch_set_features, after its own flush and after an overflow.      */
#define MP3D_FEAT_LOG10 1

/* host only, no GPU: fb[n_mels][201] floats (NULL: size only); cap = floats
 * fb can hold; returns n_mels * 201 or MP3D_E_ARG */
MP3D_API long long mp3d_mel_filterbank(int n_mels, float *fb, size_t cap);

/* host only: a feat_stride that can never overflow for one call of `frames`
 * frames per stream of input rate >= min_in_hz: ceil((S + 200) / 160) + 1
 * with S = mp3d_packed_max_samples(16000, frames, min_in_hz); 0 when S is 0 */
MP3D_API long long mp3d_feat_max_frames(int frames, int min_in_hz);

/* Needs the packed sink set to (16000, 1), else MP3D_E_ARG.  n_mels = 0 turns
 * the feature sink off and frees its buffers; flags: MP3D_FEAT_LOG10.  Uploads
 * the filterbank (per-filter bin ranges plus weights), restarts every
 * stream's feature state and waits for the handle's work. */
MP3D_API int mp3d_batch_set_features(mp3d_batch *b, int n_mels, int flags);

/* Decodes exactly as mp3d_batch_decode_packed does (decoder and resampler
 * state advance exactly so) into a handle-owned sample buffer of stride
 * mp3d_packed_max_samples(16000, frames_per_stream, 0), then stream s writes
 * feat_count[s] frames of n_mels floats at feat + s * feat_stride * n_mels;
 * nothing past them is touched.  A stream that would exceed feat_stride gets
 * feat_count[s] = -1, writes nothing and has its feature state restarted.
 * feat, feat_count and infos (may be NULL) are host or device memory; the
 * call is asynchronous when all of them are device memory, and a host feat is
 * filled by one copy per stream, as the packed call's out is.  flags:
 * MP3D_PACK_FLUSH flushes the resampler, then the features;
 * MP3D_PACK_GAPLESS as in the packed call: the frames are centred on
 * multiples of 160 samples of the windowed signal.  MP3D_E_ARG before
 * mp3d_batch_set_features.                                                  */
MP3D_API int mp3d_batch_decode_features(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                        const uint32_t *sizes, int n_streams, int frames_per_stream, float *feat,
                                        long long feat_stride, int *feat_count, int flags, mp3d_frame_info *infos,
                                        void *hip_stream);

/* The parity tap of the feature stage: feeds counts[s] (clamped to
 * [0, sample_stride]) float32 16 kHz mono samples from samples +
 * s * sample_stride per stream through the same kernels and the same
 * per-slot state; feat, feat_stride, feat_count and flags as above.  samples
 * and counts are host or device memory (a host samples array is read whole).
 * It also turns the device output of mp3d_batch_decode_long_packed (16 kHz
 * mono) into features.  Leaves the decoder and resampler state untouched.   */
MP3D_API int mp3d_batch_features(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                 int n_streams, float *feat, long long feat_stride, int *feat_count, int flags,
                                 void *hip_stream);

/* device-side microseconds of the feature stage of the last feature call;
 * needs mp3d_batch_set_timing */
MP3D_API int mp3d_batch_feature_time(mp3d_batch *b, float *us);

/* ---- loudness sink (ITU-R BS.1770-4 / EBU R128 measurement) --------------- *
 * Input signal of a stream: its packed-sink output in the handle's format
 * (out_hz, out_channels 1 or 2, float32 interleaved): x_c[0 .. N) since the
 * stream's last loudness restart.  Sample windows and MP3D_PACK_GAPLESS act
 * before it, as for the features.  A stereo -> mono map of 0.5f * (l + r) is
 * measured as it is: a mono signal reads 3.01 dB below the same signal on two
 * channels, which is BS.1770's own behaviour.
 *
 * K-weighting: two biquads per channel, coefficients computed on the host in
 * double for fs = out_hz:
 *   stage 1 (shelf): f0 = 1681.974450955533, G = 3.999843853973347 dB,
 *                    Q = 0.7071752369554196
 *     K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *     a0 = 1 + K/Q + K^2
 *     b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0
 *     a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
 *   stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773,
 *     K = tan(pi f0 / fs), a0 = 1 + K/Q + K^2
 *     b = [1, -2, 1],  a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
 * (at 48 000 Hz the BS.1770 table).  Each stage is transposed direct form II
 * in double; with v the float32 sample widened to double:
 *   o = b0 v + s1;  s1 = b1 v - a1 o + s2;  s2 = b2 v - a2 o
 * Stage 2 takes stage 1's o, and y_c is stage 2's o.
 *
 * Blocks: H = (out_hz + 5) / 10 samples (integer division), 100 ms.
 *   z[b] = sum_c (1/H) sum_{i = bH .. (b+1)H - 1} y_c[i]^2
 * accumulated in double, stored as float32.  Momentary loudness is 4 blocks,
 * short-term 30 blocks: -0.691 + 10 log10(mean z).
 *
 * Emit rule: block b is emitted once sample (b+1)H - 1 has been seen, so after
 * N samples a stream has emitted floor(N / H) blocks.  MP3D_PACK_FLUSH drops
 * the incomplete block (BS.1770 ignores incomplete blocks) and restarts the
 * stream's loudness state.  A stream that would exceed block_stride gets
 * count -1, writes nothing and restarts.
 *
 * Peak: peak[s] = max |x_c[i]| over the channels and the samples fed in this
 * call, float32, exact; 0 for an empty call.  (Sample peak, not true peak.)
 *
 * Integrated loudness of a block sequence z[0 .. n):
 *   G[j] = (z[j] + z[j+1] + z[j+2] + z[j+3]) / 4, j = 0 .. n - 4
 *   l[j] = -0.691 + 10 log10 G[j];  J1 = {j : l[j] > -70}
 *   Gamma = -0.691 + 10 log10(mean_{J1} G) - 10
 *   result = -0.691 + 10 log10(mean_{j in J1, l[j] > Gamma} G[j])
 * in double; -HUGE_VAL when n < 4 or no block passes.
 *
 * Numerical contract: a tolerance, not bits (the filter runs parallel in time
 * through its state-space form, and the order of its additions depends on
 * where a call's tiles fall).  The same call on the same state gives the same
 * bits every time.  Against the definition above evaluated in float64, with C
 * the channel count and P the largest |x| of the stream since its restart,
 *   |z - ref| <= 2^-22 ref + 1e-9 * C * P^2.
 *
 * The per-stream loudness state (a sample count, 2 x 4 doubles of filter
 * state, the open block's partial sum) lives in the handle while loudness is
 * set, not in the state blob.  It restarts where the feature state does: at
 * create, at mp3d_batch_reset, at mp3d_batch_set_state on its slot, at
 * mp3d_batch_set_output (which also turns loudness off), at
 * mp3d_batch_set_loudness, at mp3d_batch_set_window on its slot, after its
 * own flush and after an overflow.  Features and loudness may both be on.   */

/* host only, no GPU: coef[10] = b0 b1 b2 a1 a2 of stage 1, then of stage 2
 * (NULL: size only); cap = doubles coef can hold; returns 10, or MP3D_E_ARG
 * for a rate outside the nine or a short cap */
MP3D_API long long mp3d_loudness_filter(int hz, double *coef, size_t cap);

/* host only: a block_stride that can never overflow for one call of `frames`
 * frames per stream of input rate >= min_in_hz: floor((H - 1 + S) / H) with
 * S = mp3d_packed_max_samples(out_hz, frames, min_in_hz); 0 when S is 0 */
MP3D_API long long mp3d_loud_max_blocks(int out_hz, int frames, int min_in_hz);

/* Needs a packed format (mp3d_batch_set_output), else MP3D_E_ARG.  on != 0
 * uploads the coefficients and the state-transition tables of the format's
 * rate, restarts every slot's loudness state and waits for the handle's
 * work; on = 0 turns the sink off and frees its buffers. */
MP3D_API int mp3d_batch_set_loudness(mp3d_batch *b, int on);

/* The stage itself: feeds counts[s] (clamped to [0, sample_stride]) sample
 * frames from samples + s * sample_stride * out_channels per stream through
 * the slots' loudness state; stream s writes block_count[s] block energies at
 * blocks + s * block_stride, nothing past them, and peak[s] (peak may be
 * NULL).  samples and counts are host or device memory (a host samples array
 * is read whole); blocks, block_count and peak are host or device memory, the
 * call is asynchronous when all three are device memory, and a host blocks is
 * filled by one copy per stream.  Device pointers must be float-aligned, else
 * MP3D_E_ARG.  flags: MP3D_PACK_FLUSH only.  This is what a caller runs on the
 * device out and out_count of mp3d_batch_decode_packed (float32), or on the
 * device output of mp3d_batch_decode_long_packed with n_streams = 1, without
 * decoding twice.  Leaves the decoder and resampler state untouched.
 * MP3D_E_ARG before mp3d_batch_set_loudness.                                */
MP3D_API int mp3d_batch_loudness(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                 int n_streams, float *blocks, long long block_stride, int *block_count, float *peak,
                                 int flags, void *hip_stream);

/* Decodes exactly as mp3d_batch_decode_packed does (decoder and resampler
 * state advance exactly so) into a handle-owned float32 sample buffer of
 * stride mp3d_packed_max_samples(out_hz, frames_per_stream, 0) with device
 * counts, then runs the stage on it: for scanning a corpus whose PCM is not
 * wanted.  flags: MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS, both forwarded (the
 * flush ends the resampler, then drops the open block).                     */
MP3D_API int mp3d_batch_decode_loudness(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                        const uint32_t *sizes, int n_streams, int frames_per_stream, float *blocks,
                                        long long block_stride, int *block_count, float *peak, int flags,
                                        mp3d_frame_info *infos, void *hip_stream);

/* host only: the integrated loudness of z[0 .. n) as defined above */
MP3D_API int mp3d_loudness_integrated(const float *z, long long n, double *lufs);

/* The same gating on the device for n_streams rows blocks + s * block_stride
 * of counts[s] blocks each, so a normalisation gain never leaves the GPU:
 * lufs[s] as float32, -INFINITY for a count of -1 or < 4 or when no block
 * passes.  Host or device pointers, as above.  Needs mp3d_batch_set_loudness. */
MP3D_API int mp3d_batch_loudness_integrated(mp3d_batch *b, const float *blocks, long long block_stride,
                                            const int *counts, int n_streams, float *lufs, void *hip_stream);

/* device-side microseconds of the loudness stage of the last loudness call;
 * needs mp3d_batch_set_timing */
MP3D_API int mp3d_batch_loudness_time(mp3d_batch *b, float *us);

/* ---- true peak and gain (normalising on the GPU) ---------------------------- *
 * Input signal of a stream: its packed-sink output in the handle's format
 * (any of the nine rates, out_channels 1 or 2, float32 interleaved):
 * x_c[0 .. N) since the stream's last true-peak restart.
 *
 * Oversampling: R = 4 at every rate, T = 12 taps per phase; the filter is
 * defined by formula (BS.1770's Annex 2 table is not used):
 *   p = 0:     taps[0][5] = 1, every other taps[0][j] = 0   (by definition)
 *   p = 1..3:  t = p/4 - (j - 5),  j = 0 .. 11
 *              w = I0(6 sqrt(1 - (t/6)^2)) / I0(6) for |t| < 6, else 0
 *                                                        (Kaiser, beta 6)
 *              h = sinc(t) w;  taps[p][j] = h / sum_j h
 * computed in double, rounded to float32 (mp3d_truepeak_filter).
 *   u_c[4n + p] = sum_j taps[p][j] x_c[n - 5 + j],  x outside [0, N) = 0
 * Each u is ONE float32 fmaf chain in ascending j, starting from 0, so its
 * bits do not depend on which call, tile or thread computes it.  Phase 0
 * reproduces x exactly (the kernel takes |x|), so a flushed stream's true
 * peak is never below its sample peak.
 *
 * Emit rule: index n (its four values, all channels) is emitted once sample
 * n + 6 has been seen, so after N samples the indices n < max(N - 6, 0) have
 * been emitted.  MP3D_PACK_FLUSH also emits every n < N, with zeros past N,
 * then restarts the stream's true-peak state.
 *
 * tpeak[s] of a call = max |u_c[4n + p]| over c, p and the indices n the call
 * emits, float32; 0 when it emits none.  A maximum is exact: the maximum of
 * tpeak[s] over ANY split of a stream into calls equals the one-call value
 * bit for bit, and a caller folds the calls of a stream with max.
 *
 * Numerical contract: against the definition evaluated in float64 with the
 * float32 taps, with P the largest |x| of the stream since its restart,
 *   |tpeak - ref| <= 23 * 2^-24 * P
 * (12 roundings of a chain whose sum of |taps| is at most 1.856).
 *
 * The per-stream true-peak state (a sample count and the last 11 samples of
 * each channel) lives in the handle while true peak is set, not in the state
 * blob.  It restarts where the loudness state does: at create, at
 * mp3d_batch_reset, at mp3d_batch_set_state on its slot, at
 * mp3d_batch_set_output (which also turns true peak off), at
 * mp3d_batch_set_true_peak, at mp3d_batch_set_window on its slot and after
 * its own flush.  Features, loudness and true peak may all be on.
 *
 * Gain rule (mp3d_batch_normalize_gain), in double, rounded to float32:
 *   g = 10^((target_lufs - lufs[s]) / 20)
 *   if tpeak[s] > 0 and g * tpeak[s] > c, c = 10^(max_dbtp / 20):
 *       g = c / tpeak[s]
 *   lufs[s] not finite (-inf: under 400 ms or silent; NaN): g = 1 exactly,
 *   untouched by the limit.
 *
 * Apply (mp3d_batch_apply_gain): out[s][i][c] = samples[s][i][c] * gain[s],
 * one float32 multiply, for i < counts[s]; nothing past that is written.
 * int16 output is the packed sink's conversion of that product,
 * clamp(floor(y * 32768 + 0.5)); float32 is not clipped.                     */

/* host only, no GPU: taps[4][12] as defined above (NULL: size only); cap =
 * floats taps can hold; returns 48, or MP3D_E_ARG for a short cap */
MP3D_API long long mp3d_truepeak_filter(float *taps, size_t cap);

/* Needs a packed format (mp3d_batch_set_output), else MP3D_E_ARG.  on != 0
 * uploads the taps, restarts every slot's true-peak state and waits for the
 * handle's work; on = 0 turns the tap off and frees its buffers. */
MP3D_API int mp3d_batch_set_true_peak(mp3d_batch *b, int on);

/* The tap: feeds counts[s] (clamped to [0, sample_stride]) sample frames from
 * samples + s * sample_stride * out_channels per stream through the slots'
 * true-peak state and writes tpeak[s].  samples, counts and tpeak are host or
 * device memory (a host samples array is read whole); the call is
 * asynchronous when all three are device memory.  Device pointers must be
 * float-aligned, else MP3D_E_ARG; sample_stride is at most 2^31 - 1 - 4096.
 * flags: MP3D_PACK_FLUSH only.  Runs on the device out and out_count of
 * mp3d_batch_decode_packed (float32), or with n_streams = 1 on the device
 * output of mp3d_batch_decode_long_packed, whose one stream is spread over
 * the whole GPU.  Leaves decoder, resampler, feature and loudness state
 * untouched.  MP3D_E_ARG before mp3d_batch_set_true_peak.                   */
MP3D_API int mp3d_batch_true_peak(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                  int n_streams, float *tpeak, int flags, void *hip_stream);

/* Exactly mp3d_batch_decode_loudness, then the true-peak tap on the same
 * handle-owned samples and counts before returning: blocks, block_count, peak
 * as there, tpeak as above.  flags: MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS (the
 * flush ends resampler, loudness and true peak).  Needs both
 * mp3d_batch_set_loudness and mp3d_batch_set_true_peak, else MP3D_E_ARG.    */
MP3D_API int mp3d_batch_decode_measure(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                       const uint32_t *sizes, int n_streams, int frames_per_stream, float *blocks,
                                       long long block_stride, int *block_count, float *peak, float *tpeak, int flags,
                                       mp3d_frame_info *infos, void *hip_stream);

/* The gain rule above for n_streams streams: lufs, tpeak (NULL: no limit) and
 * gain are host or device memory (device pointers float-aligned); the call is
 * asynchronous when all are device memory.  Needs no sink.                 */
MP3D_API int mp3d_batch_normalize_gain(mp3d_batch *b, const float *lufs, const float *tpeak, int n_streams,
                                       double target_lufs, double max_dbtp, float *gain, void *hip_stream);

/* Applies gain[s] to counts[s] (clamped to [0, sample_stride]; < 0 writes
 * nothing) sample frames of every stream: samples as for the tap, out
 * float32 (f32 != 0) or int16 with the same stride, host or device memory.  A
 * device out must be aligned to one sample frame (as
 * mp3d_batch_decode_packed's out); a host out is filled by one copy per
 * stream.  out == samples (in place) is allowed for float32.  Needs a packed
 * format, for the channel count, else MP3D_E_ARG.                           */
MP3D_API int mp3d_batch_apply_gain(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                   int n_streams, const float *gain, void *out, int f32, void *hip_stream);

/* device-side microseconds of the true-peak stage of the last true-peak call
 * (mp3d_batch_true_peak, mp3d_batch_decode_measure); needs
 * mp3d_batch_set_timing */
MP3D_API int mp3d_batch_true_peak_time(mp3d_batch *b, float *us);

/* ---- tempo sink (pitch-preserving time stretch, WSOLA) ---------------------- *
 * Input signal of a stream: its packed-sink output in the handle's format
 * (any of the nine rates fs, C = out_channels 1 or 2, float32 interleaved):
 * x_c[0 .. N) since the stream's last stretch restart, x outside [0, N) = 0.
 * Sample windows and MP3D_PACK_GAPLESS act before it.
 *
 * Constants of the format: H = (fs + 50) / 100 in integer division (10 ms:
 * 480 at 48 kHz, 80 at 8 kHz, 110 at 11 025 Hz); D = H / 2, the search radius.
 *
 * Tempo of a slot: a rational num / den, 1 <= num, den <= 4096 and
 * 1/2 <= num/den <= 2.  The output plays num/den times as fast and has
 * M = ceil(N den / num) samples per channel.
 *
 * Crossfade table: w[n] = float32(0.5 - 0.5 cos(pi (n + 0.5) / H)), n < H,
 * computed in double (mp3d_stretch_window).
 *
 * Match signal, integers:
 *   m[i] = x_0[i] (mono), 0.5f * (x_0[i] + x_1[i]) (stereo), float32
 *   q[i] = (int) clamp(floorf(m[i] * 1024.0f + 0.5f), -1023, 1023)
 * Samples are finite; a NaN gives an unspecified result but no fault.
 *
 * Block k = 0, 1, ... is output samples [kH, (k+1)H):
 *   t_k = floor(k H num / den) (64-bit), t_{-1} = -H
 *   a_{-1} = -H;  r_k = a_{k-1} + H (where the last segment would go on)
 *   a_0 = 0;  for k >= 1, over every delta in [-D, D] with t_k + delta >= 0:
 *     d_k(delta) = sum_{n<H} (q[r_k + n] - q[t_k + delta + n])^2
 *   an exact integer that fits int32 (2046^2 * 480 < 2^31); delta_k is the
 *   delta of the smallest d_k, ties to the smallest |delta|, then to the
 *   negative one; a_k = t_k + delta_k
 *   y_c[kH + n] = x_c[r_k + n] + fl(w[n] * fl(x_c[a_k + n] - x_c[r_k + n]))
 * three separately rounded float32 operations, never fused.  Every term is
 * exact or one rounding, so the output has one value whatever call or lane
 * computes it.  At num == den every delta_k is 0 and y == x; a signal of an
 * integer period P <= 2D comes out as the same periodic signal at any tempo
 * wherever no block reads past N.
 *
 * Emit rule (data independent): block k is emitted once sample e_k has been
 * seen (N - 1 >= e_k),
 *   e_k = max(max(t_k, t_{k-1} + H) + D + H - 1, t_{k+1} - 1)
 * the first term covers every sample a candidate or r_k can read (r_k <=
 * t_{k-1} + D + H), the second keeps a whole emitted block inside M.
 * MP3D_PACK_FLUSH also emits every block with kH < M, with zeros past N, the
 * last block cut to M - kH samples: the lifetime total is exactly M; then the
 * slot's stretch state restarts.
 *
 * Overflow: a stream whose call would emit more than out_stride samples gets
 * count -1, writes nothing and restarts.  A call that feeds S samples emits at
 * most mp3d_stretch_max_samples = ceil((S + 2H + D) den / num): the next block
 * k before the call has N <= e_k, and with t_j <= jH num / den that gives
 *   N den / num - kH <= max((D + H - 1) den / num,
 *                           (2H + D - 1) den / num - H,  H) <= (2H + D) den / num
 * (den / num >= 1/2), so no more than (S + 2H + D) den / num samples of the
 * M after the call are still to be emitted.
 *
 * The per-slot stretch state (N, k, a_{k-1} and the input from max(0,
 * min(r_k, t_k - D)) on, at most 3H + D - 1 sample frames) lives in the
 * handle while stretch is set, not in the state blob.  It restarts where the
 * true-peak state does: at create, at mp3d_batch_reset, at
 * mp3d_batch_set_state on its slot, at mp3d_batch_set_output (which also
 * turns stretch off), at mp3d_batch_set_stretch, at mp3d_batch_set_window on
 * its slot, after its own flush and after an overflow; and at
 * mp3d_batch_set_tempo on its slot.                                        */

/* host only, no GPU: w[H] as defined above (NULL: size only); cap = floats w
 * can hold; returns H, or MP3D_E_ARG for a rate that is not an MPEG audio
 * rate or a short cap */
MP3D_API long long mp3d_stretch_window(int hz, float *w, size_t cap);

/* host only: an out_stride no stream can exceed in one call that feeds
 * in_samples (at most 2^31 - 1) samples at tempo num / den, whatever earlier
 * calls left pending and flushed or not: ceil((in_samples + 2H + D) den / num).
 * MP3D_E_ARG for a bad rate, count or ratio. */
MP3D_API long long mp3d_stretch_max_samples(int out_hz, long long in_samples, int num, int den);

/* Needs a packed format (mp3d_batch_set_output), else MP3D_E_ARG.  on != 0
 * uploads w, restarts every slot's stretch state, sets every slot's tempo to
 * 1/1 and waits for the handle's work; on = 0 turns the sink off and frees its
 * buffers. */
MP3D_API int mp3d_batch_set_stretch(mp3d_batch *b, int on);

/* The tempo of slots [first, first + n): num and den are host arrays.
 * Restarts those slots' stretch state and waits for the handle's work.
 * MP3D_E_ARG (nothing written) for a ratio outside the range above or before
 * mp3d_batch_set_stretch; MP3D_E_CAPACITY past max_streams. */
MP3D_API int mp3d_batch_set_tempo(mp3d_batch *b, int first, int n, const int *num, const int *den);

/* The stage: feeds counts[s] (clamped to [0, sample_stride]) sample frames
 * from samples + s * sample_stride * out_channels per stream through the
 * slots' stretch state and writes the emitted blocks to out + s * out_stride *
 * out_channels and their sample count to out_count[s] (-1: over out_stride).
 * Nothing past out_count[s] is written.  samples, counts, out and out_count
 * are host or device memory (a host samples array is read whole; a host out
 * is filled by one copy per stream); the call is asynchronous when all four
 * are device memory.  Device pointers must be element-aligned and a device out
 * aligned to one sample frame, else MP3D_E_ARG; both strides are at most
 * 2^31 - 1; out may not overlap samples (MP3D_E_ARG).  flags: MP3D_PACK_FLUSH
 * only.  Runs on the device out and out_count of mp3d_batch_decode_packed
 * (float32), or with n_streams = 1 on the device output of
 * mp3d_batch_decode_long_packed (one stream is a chain of blocks: it runs on
 * one compute unit).  Its device out and out_count are valid inputs to
 * mp3d_batch_features, mp3d_batch_loudness, mp3d_batch_true_peak and
 * mp3d_batch_apply_gain.  Leaves decoder, resampler, feature, loudness and
 * true-peak state untouched.  MP3D_E_ARG before mp3d_batch_set_stretch.     */
MP3D_API int mp3d_batch_stretch(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                int n_streams, float *out, long long out_stride, int *out_count, int flags,
                                void *hip_stream);

/* mp3d_batch_decode_packed (float32) into a handle-owned buffer of stride
 * mp3d_packed_max_samples(out_hz, frames_per_stream, 0) with device counts,
 * then the stage on them.  flags: MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS, both
 * forwarded (the flush ends the resampler, then the stretch).               */
MP3D_API int mp3d_batch_decode_stretched(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                         const uint32_t *sizes, int n_streams, int frames_per_stream, float *out,
                                         long long out_stride, int *out_count, int flags, mp3d_frame_info *infos,
                                         void *hip_stream);

/* device-side microseconds of the stretch stage of the last stretch call
 * (mp3d_batch_stretch, mp3d_batch_decode_stretched); needs
 * mp3d_batch_set_timing */
MP3D_API int mp3d_batch_stretch_time(mp3d_batch *b, float *us);

/* ---- limiter (look-ahead, true-peak detector) ------------------------------- *
 * A per-sample gain stage behind the static gain of the normalise path: the
 * gain may reach its loudness target (mp3d_batch_normalize_gain with tpeak =
 * NULL) and the limiter holds the peaks under a ceiling.
 *
 * Input signal of a slot: packed-sink output in the handle's format (any of
 * the nine rates fs, C = out_channels 1 or 2, float32 interleaved):
 * x_c[0 .. N) since the slot's last limiter restart.  Samples are finite; a
 * NaN or Inf gives an unspecified value but no fault.
 *
 * Constants: A = (fs + 50) / 100 in integer division, the look-ahead (10 ms:
 * 480 at 48 kHz, 80 at 8 kHz, 110 at 11 025 Hz); Hd = 2A, the hold; Q = 2^20;
 * the ceiling c = float32(10^(ceiling_db / 20)) computed in double,
 * -20 <= ceiling_db <= 0, one per handle.
 *
 * Pre-gain: v_c[i] = fl(x_c[i] * gain[s]), one float32 multiply with the
 * gain[s] of the call that fed sample i; a NULL gain is 1 and v is x itself;
 * v outside [0, N) = 0.
 *
 * Detector: the true-peak tap's oversampler on v.  u_c[4i + p] exactly as in
 * "true peak and gain" above (mp3d_truepeak_filter's taps, one float32 fmaf
 * chain in ascending j from 0, phase 0 is |v|);
 *   p[i] = max over c and p of |u_c[4i + p]|
 *
 * Required gain, integers from here on:
 *   r[i] = 1 if p[i] <= c, else fl(c / p[i])         (IEEE float32 division)
 *   R[i] = (int) floorf(r[i] * 1048576.0f)           (exact); R outside [0, N) = Q
 *   m[k] = min_{k - Hd <= j <= k + A} R[j]
 *   S[i] = sum_{j = 0 .. A} m[i - j]                 (fits int32: 481 * 2^20 < 2^31)
 *   G[i] = S[i] / (A + 1)                            (integer division)
 *   g[i] = (float) G[i] * 2^-20                      (exact)
 *   y_c[i] = fl(v_c[i] * g[i])
 * int16 output is the packed sink's clamp(floor(y * 32768 + 0.5)).
 *
 * What follows from it:
 *   - every m[i - j] of the sum covers index i, so g[i] <= R[i] / Q <= r[i] and
 *     |y_c[i]| <= c (1 + 2^-22) for every sample;
 *   - if p[i] <= c over a whole stream, every g is 1 and y == v bit for bit;
 *   - a peak at i0 pulls the gain down linearly over the A samples before it,
 *     holds it for Hd samples and releases it over A + 1;
 *   - the minimum and the sum are integers: any evaluation order, tile size or
 *     scan gives the same G, and any split of a stream into calls the same y;
 *   - the TRUE peak of y is not bounded by c exactly, because the gain moves
 *     between samples: it is measured, not promised.
 *
 * Emit rule: sample i is emitted once sample i + A + 6 has been seen.
 * MP3D_PACK_FLUSH also emits every i < N, with zeros past N, then restarts the
 * slot.  A slot's lifetime output count equals its input count.  A call that
 * feeds S samples emits at most S + A + 6 (mp3d_limiter_max_samples).  A
 * stream whose call would emit more than out_stride gets count -1, writes
 * nothing and restarts.
 *
 * gr[s] (optional) = the minimum g[i] over the samples the call emits, float32
 * and exact; 1 when it emits none.  A caller folds a stream's calls with min.
 *
 * Emitting i reads v[i - 3A - 5 .. i + A + 6]: the per-slot limiter state is a
 * sample count and the last 4A + 11 sample frames of v (15 456 bytes at 48 kHz
 * stereo).  It lives in the handle while the limiter is set, not in the state
 * blob, and restarts where the true-peak state does: at create, at
 * mp3d_batch_reset, at mp3d_batch_set_state on its slot, at
 * mp3d_batch_set_output (which also turns the limiter off), at
 * mp3d_batch_set_limiter, at mp3d_batch_set_window on its slot, after its own
 * flush and after an overflow.                                               */

/* host only: A at rate hz, or MP3D_E_ARG for a rate that is not an MPEG audio
 * rate */
MP3D_API long long mp3d_limiter_lookahead(int hz);

/* host only: an out_stride no stream can exceed in one call that feeds
 * in_samples (at most 2^31 - 1) samples, whatever earlier calls left pending
 * and flushed or not: in_samples + A + 6.  MP3D_E_ARG for a bad rate or count. */
MP3D_API long long mp3d_limiter_max_samples(int hz, long long in_samples);

/* Needs a packed format (mp3d_batch_set_output) and -20 <= ceiling_db <= 0,
 * else MP3D_E_ARG.  on != 0 sets the ceiling, restarts every slot's limiter
 * state and waits for the handle's work; on = 0 turns the limiter off and
 * frees its buffers. */
MP3D_API int mp3d_batch_set_limiter(mp3d_batch *b, int on, double ceiling_db);

/* The stage: feeds counts[s] (clamped to [0, sample_stride]) sample frames
 * from samples + s * sample_stride * out_channels per stream, times gain[s]
 * (gain NULL: 1), through the slots' limiter state and writes the emitted
 * samples as float32 (f32 != 0) or int16 to out + s * out_stride *
 * out_channels elements, their count to out_count[s] (-1: over out_stride)
 * and, when gr is not NULL, the call's smallest gain to gr[s].  Nothing past
 * out_count[s] is written.  samples, counts, gain, out, out_count and gr are
 * host or device memory (a host samples array is read whole; a host out is
 * filled by one copy per stream); the call is asynchronous when all of them
 * are device memory.  Device pointers must be element-aligned and a device out
 * aligned to one sample frame, else MP3D_E_ARG; both strides are at most
 * 2^31 - 1 - 8192 frames, and n_streams * ceil(min(sample_stride + A + 6,
 * out_stride) / 4096) at most (2^32 - 1) / 384, the launch's size, else
 * MP3D_E_CAPACITY; out may not overlap samples (MP3D_E_ARG).  flags:
 * MP3D_PACK_FLUSH only.  Runs on the device out and out_count of
 * mp3d_batch_decode_packed (float32), or with n_streams = 1 on the device
 * output of mp3d_batch_decode_long_packed: tiles are independent, so one long
 * stream is spread over the whole GPU.  Its float32 device out and out_count
 * are valid inputs to mp3d_batch_features, mp3d_batch_loudness,
 * mp3d_batch_true_peak and mp3d_batch_apply_gain.  Leaves decoder, resampler,
 * feature, loudness, true-peak and stretch state untouched.  MP3D_E_ARG before
 * mp3d_batch_set_limiter.                                                    */
MP3D_API int mp3d_batch_limit(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                              int n_streams, const float *gain, void *out, int f32, long long out_stride,
                              int *out_count, float *gr, int flags, void *hip_stream);

/* mp3d_batch_decode_packed (float32) into a handle-owned buffer of stride
 * mp3d_packed_max_samples(out_hz, frames_per_stream, 0) with device counts,
 * then the stage on them with gain, out, f32, out_stride, out_count and gr as
 * above.  flags: MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS, both forwarded (the
 * flush ends the resampler, then the limiter).                              */
MP3D_API int mp3d_batch_decode_limited(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                       const uint32_t *sizes, int n_streams, int frames_per_stream, const float *gain,
                                       void *out, int f32, long long out_stride, int *out_count, float *gr, int flags,
                                       mp3d_frame_info *infos, void *hip_stream);

/* device-side microseconds of the limiter stage of the last limiter call
 * (mp3d_batch_limit, mp3d_batch_decode_limited); needs mp3d_batch_set_timing */
MP3D_API int mp3d_batch_limiter_time(mp3d_batch *b, float *us);

/* ---- segment sink (speech and pause boundaries) ----------------------------- *
 * Where a sentence starts and ends: the sample ranges in which a stream's
 * short-time energy stays over a threshold, pauses shorter than a minimum
 * filled and runs shorter than a minimum dropped.
 *
 * Input signal of a slot: packed-sink output in the handle's format (any of
 * the nine rates fs, C = out_channels 1 or 2, float32 interleaved):
 * x_c[0 .. N) since the slot's last segment restart.  Sample windows and
 * MP3D_PACK_GAPLESS act before it.  Samples are finite; a NaN gives an
 * unspecified result but no fault.
 *
 * Constants: H = (fs + 50) / 100 in integer division (a hop of 10 ms, the
 * tempo sink's H: 441 at 44.1 kHz, 221 at 22 050 Hz, 110 at 11 025 Hz).  Per
 * handle, in hops: the pause P and the shortest segment S, both in [1, 256],
 * and pad with 0 <= 2 pad <= P.  Per slot: the threshold thr, an unsigned
 * 64-bit hop energy with 1 <= thr <= H * 2^30.
 *
 * Hop energy, integers after one float32 quantisation:
 *   m[i] = x_0[i] (mono), 0.5f * (x_0[i] + x_1[i]) (stereo), float32, the tempo
 *          sink's mix
 *   q[i] = (int) clamp(floor(m[i] * 32768 + 0.5), -32768, 32767), the packed
 *          sink's int16 rule: the product and the sum are exact, never rounded
 *   E[b] = sum_{n < H} q[bH + n]^2, q outside [0, N) = 0      (uint64: up to H * 2^30)
 *   a[b] = E[b] >= thr
 * B is the number of hops known: floor(N / H) before a flush, ceil(N / H) at a
 * flush (the open hop is completed with zeros).  a outside [0, B) is 0.
 *
 * Masks:
 *   c[b] = 1 iff there are i <= b <= j with a[i] = a[j] = 1 and j - i <= P
 *   o[b] = 1 iff there is t with t <= b <= t + S - 1 and c[t .. t + S - 1] all 1
 * In this order: a pause of fewer than P hops between two active hops is
 * filled (leading and trailing silence never is), then a run of fewer than S
 * hops is dropped.  So a run of o is at least S hops long, and two runs are at
 * least P hops apart.
 *
 * Segments: each maximal run [b0, b1) of o is one segment,
 *   start = max(b0 - pad, 0) * H,  end = min((b1 + pad) * H, N)
 * both long long, in samples since the slot's restart.  With 2 pad <= P padded
 * segments never overlap.
 *
 * Emit rule: o[b] depends on a[b - S + 1 - P .. b + S - 1 + P] and on nothing
 * else, so it is final once b <= B - S - P.  A segment is emitted by the call
 * after which b1 <= B - S - P, that is, once sample (b1 + S + P) H - 1 has been
 * seen.  MP3D_PACK_FLUSH emits every remaining segment, an open one closed at
 * b1 = B with end = N; then the slot restarts.  The min with N acts at a flush
 * only, so any split of a stream into calls emits the same list.
 *
 * Bound: the end edges b1 a call decides lie in a range of at most K + S + P
 * hop indices, K = ceil((in_samples + H - 1) / H) being the most hops the call
 * can complete, the pending part hop included: (B0 - S - P, B1 - S - P] with
 * B1 - B0 <= K without a flush, (B0 - S - P, B1] with one.  Two end edges are
 * at least S + P apart (a run, then a gap).  So a call emits at most
 * 1 + (K + S + P - 1) / (S + P) <= mp3d_segment_max = 2 + K / (S + P) segments,
 * in integer division.
 *
 * Overflow: a slot whose call would emit more than seg_stride segments gets
 * count -1, writes nothing and restarts.
 *
 * The per-slot segment state (N, the open hop's partial energy, an integer and
 * so exact under any split, the last 1024 = 2 (S + P) bits of a at P = S = 256,
 * and the last rising edge of o: 152 bytes) lives in the handle while the sink
 * is set, not in the state blob.  It restarts where the limiter's does: at
 * create, at mp3d_batch_reset, at mp3d_batch_set_state on its slot, at
 * mp3d_batch_set_output (which also turns the sink off), at
 * mp3d_batch_set_segments, at mp3d_batch_set_window on its slot, after its own
 * flush and after an overflow; and at mp3d_batch_set_segment_threshold on its
 * slots.  The threshold outlives a restart, as the tempo does.               */

/* host only: the hop energy of a mean square of db dBFS at rate hz,
 * max(1, ceil(H * 2^30 * 10^(db / 10))) computed in double, -96 <= db <= 0;
 * MP3D_E_ARG for another db or a rate that is not an MPEG audio rate */
MP3D_API long long mp3d_segment_threshold(int hz, double db);

/* host only: a seg_stride no slot can exceed in one call that feeds in_samples
 * (at most 2^31 - 1) samples, whatever earlier calls left pending and flushed
 * or not: 2 + K / (speech_hops + pause_hops), K = ceil((in_samples + H - 1) / H).
 * MP3D_E_ARG for a bad rate, count or number of hops. */
MP3D_API long long mp3d_segment_max(int hz, long long in_samples, int pause_hops, int speech_hops);

/* Needs a packed format (mp3d_batch_set_output), pause_hops and speech_hops in
 * [1, 256] and 0 <= 2 pad_hops <= pause_hops, else MP3D_E_ARG.  on != 0 sets
 * P, S and pad, every slot's threshold to mp3d_segment_threshold(fs, -40.0),
 * restarts every slot's segment state and waits for the handle's work; on = 0
 * turns the sink off and frees its buffers. */
MP3D_API int mp3d_batch_set_segments(mp3d_batch *b, int on, int pause_hops, int speech_hops, int pad_hops);

/* The threshold of slots [first, first + n): thr is a host array.  Restarts
 * those slots' segment state and waits for the handle's work.  MP3D_E_ARG
 * (nothing written) for a threshold outside [1, H * 2^30] or before
 * mp3d_batch_set_segments; MP3D_E_CAPACITY past max_streams. */
MP3D_API int mp3d_batch_set_segment_threshold(mp3d_batch *b, int first, int n, const unsigned long long *thr);

/* The stage: feeds counts[s] (clamped to [0, sample_stride]) sample frames
 * from samples + s * sample_stride * out_channels per stream through the
 * slots' segment state and writes the segments the call emits as (start, end)
 * pairs to seg + s * seg_stride * 2 and their number to seg_count[s] (-1: over
 * seg_stride).  Nothing past seg_count[s] pairs is written.  samples, counts,
 * seg and seg_count are host or device memory (a host samples array is read
 * whole; a host seg is filled by one copy per stream); the call is
 * asynchronous when all four are device memory.  Device pointers must be
 * element-aligned (a device seg to 8 bytes), else MP3D_E_ARG; sample_stride is
 * at most 2^31 - 1 - 960 and seg_stride at most 2^31 - 1, and n_streams *
 * ceil(K / 64) at most (2^32 - 1) / 256, the launch's size, else
 * MP3D_E_CAPACITY.  flags: MP3D_PACK_FLUSH only.  Runs on the device out and
 * out_count of mp3d_batch_decode_packed (float32), of mp3d_batch_stretch or of
 * mp3d_batch_limit, or with n_streams = 1 on the device output of
 * mp3d_batch_decode_long_packed: the energy tiles are independent, so one long
 * stream is spread over the whole GPU.  Leaves decoder, resampler and every
 * other sink's state untouched.  MP3D_E_ARG before mp3d_batch_set_segments.  */
MP3D_API int mp3d_batch_segments(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                 int n_streams, long long *seg, long long seg_stride, int *seg_count, int flags,
                                 void *hip_stream);

/* mp3d_batch_decode_packed (float32) into a handle-owned buffer of stride
 * mp3d_packed_max_samples(out_hz, frames_per_stream, 0) with device counts,
 * then the stage on them.  flags: MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS, both
 * forwarded (the flush ends the resampler, then the segments).              */
MP3D_API int mp3d_batch_decode_segments(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                        const uint32_t *sizes, int n_streams, int frames_per_stream, long long *seg,
                                        long long seg_stride, int *seg_count, int flags, mp3d_frame_info *infos,
                                        void *hip_stream);

/* device-side microseconds of the segment stage of the last segment call
 * (mp3d_batch_segments, mp3d_batch_decode_segments); needs
 * mp3d_batch_set_timing */
MP3D_API int mp3d_batch_segment_time(mp3d_batch *b, float *us);

/* ---- equaliser sink (biquad cascade) ---------------------------------------- *
 * Tone control between the decoder and the limiter: a graphic EQ, a rumble
 * high-pass, a shelf.  In a player's chain: decode -> packed -> EQ -> gain ->
 * limiter.
 *
 * Input signal of a slot: packed-sink output in the handle's format (any of
 * the nine rates fs, C = out_channels 1 or 2, float32 interleaved): x_c[0 .. N)
 * since the slot's last equaliser restart.  Sample windows and
 * MP3D_PACK_GAPLESS act before it.  Samples are finite; a NaN gives an
 * unspecified result but no fault.
 *
 * Curve: one per handle, K = n_bands in [1, MP3D_EQ_MAX_BANDS] second-order
 * sections, applied to every channel of every stream in the order given.  A
 * section is designed on the host in long double by the Audio EQ Cookbook
 * (R. Bristow-Johnson) formulas in their Q form, with w0 = 2 pi f0_hz / fs,
 * alpha = sin w0 / (2 q), A = 10^(gain_db / 40), cs = cos w0, and for the
 * shelves sq = 2 sqrt(A) alpha:
 *   MP3D_EQ_PEAK        b = 1 + alpha A, -2 cs, 1 - alpha A
 *                       a = 1 + alpha / A, -2 cs, 1 - alpha / A
 *   MP3D_EQ_LOW_SHELF   b = A ((A+1) - (A-1) cs + sq), 2A ((A-1) - (A+1) cs), A ((A+1) - (A-1) cs - sq)
 *                       a = (A+1) + (A-1) cs + sq, -2 ((A-1) + (A+1) cs), (A+1) + (A-1) cs - sq
 *   MP3D_EQ_HIGH_SHELF  b = A ((A+1) + (A-1) cs + sq), -2A ((A-1) + (A+1) cs), A ((A+1) + (A-1) cs - sq)
 *                       a = (A+1) - (A-1) cs + sq, 2 ((A-1) - (A+1) cs), (A+1) - (A-1) cs - sq
 *   MP3D_EQ_HIGH_PASS   b = (1 + cs) / 2, -(1 + cs), (1 + cs) / 2;  a = 1 + alpha, -2 cs, 1 - alpha
 *   MP3D_EQ_LOW_PASS    b = (1 - cs) / 2, 1 - cs, (1 - cs) / 2;     a = 1 + alpha, -2 cs, 1 - alpha
 * gain_db is not used by the two pass types (it is still range-checked).  With
 * g = 10^(preamp_db / 20) for stage 1 and g = 1 for the others, a stage's
 * coefficients are b0 g / a0, b1 g / a0, b2 g / a0, a1 / a0, a2 / a0, each
 * evaluated in long double in that order and rounded once to double.
 *
 * Accepted (else MP3D_E_ARG, nothing changed): type one of the five, f0_hz in
 * [20, 0.45 fs], q in [0.1, 16], gain_db and preamp_db in [-24, 24].
 *
 * Arithmetic, per channel: v = the float32 sample widened to double; each stage
 * is transposed direct form II in double,
 *   o = b0 v + s1;  s1 = b1 v - a1 o + s2;  s2 = b2 v - a2 o
 * stage k + 1 takes stage k's o, and the last stage's o is rounded once to
 * float32.  It is not clipped: the limiter exists for that.
 *
 * Sample counts: the stage emits exactly as many sample frames as it is fed:
 * no latency, no tail, and a flush emits nothing extra.
 *
 * Numerical contract: a tolerance, not bits, for the loudness sink's reason
 * (the stage runs parallel in time; where a call's tiles fall decides the
 * order of additions).  The same call on the same state gives the same bits
 * every time.  With ref the definition above evaluated sequentially in float64
 * and G the largest |ref| of the stream and channel since its restart, up to
 * and including the sample,
 *   |y - ref| <= 2^-22 |ref| + eps G,   eps = 1.32e-10
 * the first term the float32 rounding of the result (factor 4), eps four times
 * the largest error over G of a float64 restatement of the time-parallel form
 * against a long double evaluation (tests/_eq.py).
 *
 * The per-slot equaliser state (2 channels x 2 K doubles, 320 bytes reserved)
 * lives in the handle while the equaliser is set, not in the state blob.  All
 * zero is a restarted stream.  It restarts where the limiter's does: at
 * create, at mp3d_batch_reset, at mp3d_batch_set_state on its slot, at
 * mp3d_batch_set_output (which also turns the equaliser off), at
 * mp3d_batch_set_eq, at mp3d_batch_set_window on its slot, after its own
 * MP3D_PACK_FLUSH and after an overflow.                                     */
#define MP3D_EQ_MAX_BANDS 10
#define MP3D_EQ_PEAK 0
#define MP3D_EQ_LOW_SHELF 1
#define MP3D_EQ_HIGH_SHELF 2
#define MP3D_EQ_HIGH_PASS 3
#define MP3D_EQ_LOW_PASS 4
typedef struct {
    int type;                 /* MP3D_EQ_*                 */
    double f0_hz, gain_db, q;
} mp3d_eq_band;

/* host only: the n_bands sections of a curve at rate hz,
 * coef[5k .. 5k + 4] = b0 b1 b2 a1 a2 of stage k (a0 = 1).  coef NULL: the
 * size only.  Returns 5 n_bands.  MP3D_E_ARG for a rate that is not an MPEG
 * audio rate, cap < 5 n_bands, n_bands outside [1, MP3D_EQ_MAX_BANDS] or any
 * field outside its range. */
MP3D_API long long mp3d_eq_design(int hz, const mp3d_eq_band *bands, int n_bands, double preamp_db, double *coef,
                                  size_t cap);

/* Needs a packed format (mp3d_batch_set_output), else MP3D_E_ARG.  n_bands > 0
 * designs the curve for the format's rate, uploads its coefficients and
 * transition tables, restarts every slot's equaliser state and waits for the
 * handle's work; n_bands = 0 turns the equaliser off and frees its buffers.
 * After MP3D_E_ARG nothing has changed. */
MP3D_API int mp3d_batch_set_eq(mp3d_batch *b, const mp3d_eq_band *bands, int n_bands, double preamp_db);

/* The stage: feeds counts[s] (clamped to [0, sample_stride]) sample frames
 * from samples + s * sample_stride * out_channels per stream through the
 * slots' equaliser state and writes as many float32 sample frames to out + s *
 * out_stride * out_channels, their count to out_count[s]; a slot whose count
 * exceeds out_stride gets -1, writes nothing and restarts.  Nothing past
 * out_count[s] is written.  samples, counts, out and out_count are host or
 * device memory (a host samples array is read whole; a host out is filled by
 * one copy per stream); the call is asynchronous when all four are device
 * memory.  Device samples and out must be aligned to one sample frame, device
 * counts to their element, else MP3D_E_ARG; both strides are at most 2^31 - 1,
 * and n_streams * ceil(min(sample_stride, out_stride) / 4096) at most
 * (2^32 - 1) / 256, the launch's size, else MP3D_E_CAPACITY; out may not
 * overlap samples (MP3D_E_ARG).  flags: MP3D_PACK_FLUSH only (the slots
 * restart after the call).  Runs on the device out and out_count of
 * mp3d_batch_decode_packed (float32), or with n_streams = 1 on the device
 * output of mp3d_batch_decode_long_packed: the tiles are independent but for a
 * small carry, so one long stream is spread over the whole GPU.  Its float32
 * device out and out_count are valid inputs to every other stage.  Leaves
 * decoder, resampler and every other sink's state untouched.  MP3D_E_ARG
 * before mp3d_batch_set_eq. */
MP3D_API int mp3d_batch_eq(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                           int n_streams, float *out, long long out_stride, int *out_count, int flags,
                           void *hip_stream);

/* mp3d_batch_decode_packed (float32) into a handle-owned buffer of stride
 * mp3d_packed_max_samples(out_hz, frames_per_stream, 0) with device counts,
 * then the stage on them.  flags: MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS, both
 * forwarded (the flush ends the resampler, then the equaliser).             */
MP3D_API int mp3d_batch_decode_equalized(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                         const uint32_t *sizes, int n_streams, int frames_per_stream, float *out,
                                         long long out_stride, int *out_count, int flags, mp3d_frame_info *infos,
                                         void *hip_stream);

/* device-side microseconds of the equaliser stage of the last equaliser call
 * (mp3d_batch_eq, mp3d_batch_decode_equalized); needs mp3d_batch_set_timing */
MP3D_API int mp3d_batch_eq_time(mp3d_batch *b, float *us);

/* ---- pitch sink (F0 contour per 10 ms hop, YIN) ----------------------------- *
 * The fundamental frequency of the voice, a record per 10 ms: what a player
 * draws as a sentence's intonation contour and what a speech pipeline takes
 * next to the log-mel frames.  The method is YIN (de Cheveigne and Kawahara,
 * JASA 111 (4), 2002): difference function, cumulative-mean normalisation,
 * absolute threshold, parabolic refinement; no smoothing across frames.
 *
 * Input signal of a slot: packed-sink output in the handle's format (any of
 * the nine rates fs, C = out_channels 1 or 2, float32 interleaved):
 * x_c[0 .. N) since the slot's last pitch restart.  Sample windows and
 * MP3D_PACK_GAPLESS act before it.  As in the segment sink:
 *   m[i] = x_0[i] (mono), 0.5f * (x_0[i] + x_1[i]) (stereo), the tempo sink's mix
 *   q[i] = (int) clamp(floor(m[i] * 32768 + 0.5), -32768, 32767), the packed
 *          sink's int16 rule; q outside [0, N) is 0
 *
 * Constants: H = (fs + 50) / 100 in integer division, W = 2 H.  Per handle:
 * integers fmin_hz and fmax_hz with 50 <= fmin_hz < fmax_hz <= 2000 and
 * 4 fmax_hz <= fs, and the threshold theta in units of 1/1024, 1 <= theta <=
 * 1024.  tmin = ceil(fs / fmax_hz), tmax = floor(fs / fmin_hz), so 4 <= tmin and
 * tmax <= 960; T = tmax + 1; SPAN = W + T, at most 1921.  Limits so close that
 * no whole lag lies between them (11 025 Hz, 1999 and 2000: tmin 6, tmax 5) are
 * accepted and leave every frame unvoiced.
 *
 * Frame f (f = 0, 1, ...) reads x_f[i] = q[f H + i], 0 <= i < SPAN.
 *  1. Block floating point: mx = max |x_f[i]|, sh = max(0, bitlen(mx) - 10) with
 *     bitlen(0) = 0, r[i] = x_f[i] >> sh (arithmetic).  Then |r| <= 1024, every
 *     cross sum over W <= 960 samples stays under 2^30 and every D under 2^32.
 *  2. For tau = 1 .. T: D(tau) = sum_{j < W} (r[j] - r[j + tau])^2, which is
 *     Q[W] + (Q[tau + W] - Q[tau]) - 2 X(tau) with Q the prefix sum of r^2 and
 *     X(tau) = sum_{j < W} r[j] r[j + tau]; S(tau) = sum_{k <= tau} D(k).
 *  3. t0 is the smallest tau in [tmin, tmax] with D(tau) * tau * 1024 <
 *     theta * S(tau): the cumulative-mean-normalised difference under
 *     theta / 1024; both sides stay under 2^53.  Without such a tau the frame
 *     is unvoiced and its record is {0.0f, 0.0f, 0, sh}.
 *  4. t starts at t0; while t < tmax and D(t + 1) < D(t), t advances: the walk
 *     to the local minimum of D (not of the normalised function, whose
 *     comparison would need 128-bit products).
 *  5. In double, with a = D(t - 1), b = D(t), c = D(t + 1) and den = a - 2 b + c
 *     formed in int64: delta = den > 0 ? 0.5 * (double)(a - c) / (double)den : 0,
 *     clamped to [-1, 1]; f0_hz = (float)(fs / (t + delta)); periodicity =
 *     (float)max(0, 1 - (double)(b * t) / (double)S(t)).  Every operand is an
 *     exactly represented integer, every operation one IEEE double operation,
 *     none a contracted multiply-add.
 *
 * Emit rule: after N samples floor((N - SPAN) / H) + 1 frames are known (0 if
 * N < SPAN); a call emits those that became known.  MP3D_PACK_FLUSH emits every
 * frame with f H < N, ceil(N / H) in all, with zeros behind N; then the slot
 * restarts.  A call that feeds in_samples emits at most mp3d_pitch_max_frames
 * = (in_samples + SPAN + H - 2) / H frames, flushed or not and whatever was
 * pending (the bound is reached).  Any split of a stream into calls gives the
 * same records, bit for bit.
 *
 * Overflow: a slot whose call would emit more than pitch_stride frames gets
 * count -1, writes nothing and restarts.
 *
 * The per-slot pitch state (N and the last min(N, SPAN - 1) <= 1920 values of
 * q as int16) lives in the handle while the sink is set, not in the state
 * blob.  All zero is a restarted stream.  It restarts where the segment
 * sink's does: at create, at mp3d_batch_reset, at mp3d_batch_set_state on its
 * slot, at mp3d_batch_set_output (which also turns the sink off), at
 * mp3d_batch_set_pitch, at mp3d_batch_set_window on its slot, after its own
 * flush and after an overflow.                                               */
typedef struct {
    float f0_hz;       /* fs / (lag + delta); 0 in an unvoiced frame            */
    float periodicity; /* 1 - the normalised difference at lag, in [0, 1]       */
    int32_t lag;       /* t in samples; 0 in an unvoiced frame                  */
    int32_t shift;     /* sh of the frame's block floating point                */
} mp3d_pitch_frame;

/* host only: SPAN at rate hz for the limits, and tmin and tmax through the
 * pointers (either may be null).  MP3D_E_ARG for a rate that is not an MPEG
 * audio rate or for limits outside the rules above. */
MP3D_API long long mp3d_pitch_span(int hz, int fmin_hz, int fmax_hz, int *tau_min, int *tau_max);

/* host only: a pitch_stride no slot can exceed in one call that feeds
 * in_samples (0 .. 2^31 - 1) samples: (in_samples + SPAN + H - 2) / H.
 * MP3D_E_ARG for a bad rate or count, or an fmin_hz that no fmax_hz fits. */
MP3D_API long long mp3d_pitch_max_frames(int hz, long long in_samples, int fmin_hz);

/* Needs a packed format (mp3d_batch_set_output) and limits inside the rules
 * above, else MP3D_E_ARG.  on != 0 sets the parameters, restarts every slot's
 * pitch state and waits for the handle's work; on = 0 turns the sink off and
 * frees its buffers. */
MP3D_API int mp3d_batch_set_pitch(mp3d_batch *b, int on, int fmin_hz, int fmax_hz, int theta);

/* The stage: feeds counts[s] (clamped to [0, sample_stride]) sample frames
 * from samples + s * sample_stride * out_channels per stream through the
 * slots' pitch state and writes the records the call emits to pitch + s *
 * pitch_stride and their number to pitch_count[s] (-1: over pitch_stride).
 * Nothing past pitch_count[s] records is written.  samples, counts, pitch and
 * pitch_count are host or device memory (a host samples array is read whole; a
 * host pitch is filled by one copy per stream); the call is asynchronous when
 * all four are device memory.  Device pointers must be element-aligned (a
 * device pitch to 8 bytes), else MP3D_E_ARG; sample_stride is at most 2^31 - 1
 * - 960 and pitch_stride at most 2^31 - 1, and n_streams * ceil(bound / 8) at
 * most (2^32 - 1) / 256, the launch's size, else MP3D_E_CAPACITY.  flags:
 * MP3D_PACK_FLUSH only.  Runs on the device out and out_count of
 * mp3d_batch_decode_packed (float32), of mp3d_batch_stretch, mp3d_batch_limit
 * or mp3d_batch_eq, or with n_streams = 1 on the device output of
 * mp3d_batch_decode_long_packed: frames are independent, so one long stream is
 * spread over the whole GPU.  Leaves decoder, resampler and every other sink's
 * state untouched.  MP3D_E_ARG before mp3d_batch_set_pitch.                   */
MP3D_API int mp3d_batch_pitch(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                              int n_streams, mp3d_pitch_frame *pitch, long long pitch_stride, int *pitch_count,
                              int flags, void *hip_stream);

/* mp3d_batch_decode_packed (float32) into a handle-owned buffer of stride
 * mp3d_packed_max_samples(out_hz, frames_per_stream, 0) with device counts,
 * then the stage on them.  flags: MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS, both
 * forwarded (the flush ends the resampler, then the pitch frames).          */
MP3D_API int mp3d_batch_decode_pitch(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                     const uint32_t *sizes, int n_streams, int frames_per_stream,
                                     mp3d_pitch_frame *pitch, long long pitch_stride, int *pitch_count, int flags,
                                     mp3d_frame_info *infos, void *hip_stream);

/* device-side microseconds of the pitch stage of the last pitch call
 * (mp3d_batch_pitch, mp3d_batch_decode_pitch); needs mp3d_batch_set_timing */
MP3D_API int mp3d_batch_pitch_time(mp3d_batch *b, float *us);

/* ---- diagnostics -------------------------------------------------------- */
MP3D_API const char *mp3d_strerror(int err);
MP3D_API int mp3d_last_hip_error(void);
MP3D_API int mp3d_abi_version(void);
/* device-side microseconds of each pipeline kernel in the last batch call
 * (demux, huffman, synth); needs mp3d_batch_set_timing(b, 1).               */
MP3D_API int mp3d_batch_set_timing(mp3d_batch *b, int enable);
MP3D_API int mp3d_batch_kernel_times(mp3d_batch *b, float *us3);

#ifdef __cplusplus
}
#endif
#endif /* MP3D_H */
