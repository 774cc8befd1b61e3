/*
 * mp3d_resample.h -- data layout of the packed uniform-rate PCM sink, shared
 * by mp3d_resample.hip and the host library ("Packed PCM sink").
 *
 * A packed call decodes float32 rows [n][F][2304] into a handle-owned buffer
 * and then runs three kernels on them:
 *   k_rs_plan    thread / stream : input count, window, first output, output count
 *   k_rs_filter  block / (stream, output tile) : channel map + polyphase FIR
 *   k_rs_update  block / stream  : history, position and fed count for the next call
 */
#ifndef MP3D_RESAMPLE_H
#define MP3D_RESAMPLE_H

#include <stdint.h>

#define MP3D_RS_RATES 9
#define MP3D_RS_MAX_TAPS 288  /* 48 kHz -> 8 kHz */
#define MP3D_RS_HIST 288      /* history samples kept per channel (>= taps - 1) */
#define MP3D_RS_SPAN 4096     /* input samples per channel one filter block stages */
#define MP3D_RS_THREADS 256
#define MP3D_RS_UP_TAPS 48    /* taps per phase of every upsampling filter */

/* Per-stream resampler state (one per stream slot of the handle; NOT part of
 * the StreamState blob).  All zero = restarted, window not fixed.
 *
 * The window: r counts the input samples per channel the slot was fed since
 * its window restart, kept or not; sample r reaches the channel map and the
 * filter only when lo <= r < hi.  The resampler (pos, hist) sees the kept
 * samples as one contiguous signal.  A flush or an overflow restarts the
 * resampler (rate_i, pos, hist) and leaves fixed, lo, hi and r alone.  The
 * host writes the first three words through RsWindow. */
struct RsState {
    int32_t rate_i;  /* 1 + index of the stream's input rate; 0: none yet      */
    int32_t fixed;   /* the window is fixed: lo, hi hold it (else [0, no end)) */
    int64_t lo, hi;  /* the window, hi = INT64_MAX: no end                     */
    int64_t r;       /* samples fed since the window restart                   */
    /* kept input samples since the restart, reduced by multiples of M once
     * past post + M (outputs then shift by multiples of L: every relative
     * index and phase is unchanged), so it never grows                       */
    int64_t pos;
    float hist[MP3D_RS_HIST * 2]; /* last pre + post channel-mapped kept inputs,
                                   * interleaved by output channel, oldest first */
};

/* the head of RsState as mp3d_batch_set_window writes it and
 * mp3d_batch_sink_window reads it (with r behind it) */
struct RsWindow {
    int32_t rate_i, fixed;
    int64_t lo, hi;
};

/* One polyphase filter of the handle's output rate (input rate index i). */
struct RsFilt {
    int32_t L, M, T;   /* phases, decimation, taps per phase (1, 1, 1: bypass)  */
    int32_t Tp;        /* device row stride in floats (T rounded up to 4)       */
    int32_t pre, post; /* inputs before / after n0 an output reads              */
    int32_t off;       /* float offset of taps[L][Tp] in the device table       */
    int32_t tile;      /* outputs per filter block                              */
    int32_t S;         /* output stride of one thread: a multiple of L when the
                        * taps stay in registers (T == 48), else the block size */
};

struct RsCfg {
    RsFilt f[MP3D_RS_RATES];
    int32_t out_ch;
};

/* Per-stream plan of one call (k_rs_plan -> k_rs_filter, k_rs_update).  The
 * call's fed samples [0, fed) split into skip before the window, n_in kept,
 * and the rest past it; kept sample rel is sample rel + skip of the prefix. */
struct RsPlan {
    int64_t pos;     /* state position at the call's start                     */
    int64_t m0;      /* first output index of the call                         */
    int32_t rate_i;  /* 1 + input rate index, 0: the stream has no audio yet   */
    int32_t n_in;    /* kept input samples of the call                         */
    int32_t count;   /* outputs of the call; -1: over the stride               */
    int32_t restart; /* the resampler restarts after the call (flush, overflow) */
    int32_t skip;    /* samples of the call before the window                  */
    int32_t fed;     /* samples fed by the call, kept or not                   */
};

/* prefix[s * (F + 1) + f]: samples fed by the call before frame f */

/*
 * The long-stream sink (mp3d_batch_decode_long_packed): ONE stream, decoded
 * in chunks of virtual streams; after each chunk's decode three kernels run
 * on the chunk's segment rows [ns][F][2304] in place (no gathered rows):
 *   k_rsl_plan    one block : prefix sum of the chunk's output frames' input
 *                             samples (block scan per stride), rate, trim
 *                             window, the chunk's outputs [m0, m1)
 *   k_rsl_filter  block / output tile of the chunk : as k_rs_filter, input
 *                             found through the prefix in the segments' rows
 *   k_rsl_carry   one block : the last T - 1 inputs and the counts
 * All positions are 64-bit and absolute: r counts the stream's inputs before
 * the trim, q = r - lo those after it (the resampler's time axis), m outputs.
 */
struct RsLong {
    int64_t raw;     /* inputs before the trim seen by earlier chunks          */
    int64_t lo, hi;  /* trim window: inputs r in [lo, hi) are kept             */
    int64_t q0, q1;  /* plan: trimmed inputs before / through this chunk       */
    int64_t m0, m1;  /* plan: outputs [m0, m1) of this chunk; m1 carries over  */
    int32_t rate_i;  /* 1 + input rate index, 0: no audio yet                  */
    int32_t n_in;    /* plan: the chunk's inputs before the trim               */
    float hist[MP3D_RS_HIST * 2]; /* inputs q0 - (T - 1) .. q0 - 1, as RsState  */
};
/* All zero = the stream's start.  lprefix[jl], jl <= n_out: the chunk's
 * inputs (before the trim) before its output frame jl, in gather order. */

#endif
