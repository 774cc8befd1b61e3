/*
 * mp3d_normalize.h -- data layout of the true-peak tap and the gain kernels,
 * shared by mp3d_normalize.hip and the host library (include/mp3d.h "true
 * peak and gain").
 *
 * A true-peak call has a stream's new float32 samples (1 or 2 channels,
 * interleaved) contiguous in device memory and runs three kernels on them:
 *   k_tp_plan    thread / stream : samples before, clamped count, first and
 *                last emitted index, tile count, restart flag
 *   k_tp_peak    block / (stream, tile of MP3D_TP_TILE emitted indices) : the
 *                tile's span and its halo (history from TpState, zeros past a
 *                flushed end) into LDS as interleaved sample frames, every
 *                thread slides a register window over MP3D_TP_SEG consecutive
 *                indices, three 12-tap FMA chains and |x| per index and
 *                channel (a stereo frame's two chains in one packed FMA), wave
 *                and block maximum
 *   k_tp_finish  wave / stream   : maximum over the tiles, tpeak[s], the new
 *                TpState
 * k_gain_calc (thread / stream) is the gain rule and k_gain_apply (block /
 * (stream, chunk of MP3D_GA_CHUNK elements)) multiplies packed samples by
 * their stream's gain into float32 or int16.
 */
#ifndef MP3D_NORMALIZE_H
#define MP3D_NORMALIZE_H

#include <stdint.h>

#define MP3D_TP_R 4                                   /* oversampling factor                 */
#define MP3D_TP_TAPS 12                               /* taps per phase                      */
#define MP3D_TP_PRE 5                                 /* index n reads x[n - PRE ..           */
#define MP3D_TP_POST 6                                /*                  .. n + POST]        */
#define MP3D_TP_HIST (MP3D_TP_TAPS - 1)               /* samples carried between calls       */
#define MP3D_TP_THREADS 256
#define MP3D_TP_SEG 16                                /* emitted indices one thread computes */
#define MP3D_TP_TILE 4096                             /* emitted indices one block computes: THREADS * SEG */
/* a run of SEG sample frames in LDS: an odd stride in frames, so the lanes of a read hit distinct banks */
#define MP3D_TP_PAD (MP3D_TP_SEG + 1)
/* a tile's span is TILE + HIST samples: that many runs of SEG, the last one partial */
#define MP3D_TP_RUNS ((MP3D_TP_TILE + MP3D_TP_HIST + MP3D_TP_SEG - 1) / MP3D_TP_SEG)
#define MP3D_GA_THREADS 256
#define MP3D_GA_CHUNK 8192                            /* elements (samples x channels) one block scales */

/* Per-stream true-peak state (one per stream slot of the handle, only while
 * true peak is set; NOT part of the StreamState blob).  All zero = restarted. */
struct TpState {
    int64_t n;                   /* samples since the restart                              */
    float hist[2][MP3D_TP_HIST]; /* per channel x[n - 11 .. n - 1], zeros before the start */
};

/* Per-stream plan of one call (k_tp_plan -> the other kernels). */
struct TpPlan {
    int64_t n0;      /* samples seen before the call                       */
    int64_t e0;      /* first index the call emits                         */
    int32_t n_in;    /* samples of the call                                */
    int32_t n_emit;  /* indices the call emits: [e0, e0 + n_emit)          */
    int32_t tiles;   /* ceil(n_emit / MP3D_TP_TILE)                        */
    int32_t restart; /* the state restarts after the call (flush)          */
};

#endif
