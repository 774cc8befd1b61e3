/*
 * mp3d_features.h -- data layout of the log-mel feature sink, shared by
 * mp3d_features.hip and the host library (include/mp3d.h "log-mel feature
 * sink").
 *
 * A feature call has a stream's new 16 kHz mono float32 samples contiguous in
 * device memory (the packed sink's output, or the caller's for the tap) and
 * runs three kernels on them:
 *   k_ft_plan       thread / stream : first frame, frame count or -1
 *   k_ft_transform  block / (stream, tile of frames) : window, 200-point
 *                   complex FFT of the packed real frame, unpack, power, mel
 *   k_ft_update     block / stream  : carry and sample count for the next call
 */
#ifndef MP3D_FEATURES_H
#define MP3D_FEATURES_H

#include <stdint.h>

#define MP3D_FT_WIN 400     /* samples per frame (25 ms at 16 kHz)              */
#define MP3D_FT_HOP 160     /* samples between frame centres (10 ms)            */
#define MP3D_FT_HALF 200    /* a frame starts this many samples before its centre */
#define MP3D_FT_BINS 201    /* power spectrum bins k = 0 .. 200                 */
#define MP3D_FT_MAX_MELS 128
#define MP3D_FT_TILE 16     /* frames per transform block                       */
#define MP3D_FT_THREADS 256
/* samples one transform block stages: TILE hops + the last frame's remainder */
#define MP3D_FT_SPAN (MP3D_FT_TILE * MP3D_FT_HOP + MP3D_FT_WIN - MP3D_FT_HOP)
/* no bin lies in more than two filters: the weights of all filters together */
#define MP3D_FT_MAX_WTS (2 * MP3D_FT_BINS + 2)

/* Per-stream feature state (one per stream slot of the handle, only while
 * features are set; NOT part of the StreamState blob).  All zero = restarted.
 * With t the next frame to emit, carry[i] is sample max(0, 160 t - 200) + i of
 * the stream, up to its last sample seen: at most 399 of them. */
struct FtState {
    int64_t n; /* samples since the restart */
    float carry[MP3D_FT_WIN];
};

/* Per-stream plan of one call (k_ft_plan -> k_ft_transform, k_ft_update). */
struct FtPlan {
    int64_t n0;      /* samples seen before the call                           */
    int64_t t0;      /* first frame of the call                                */
    int32_t n_in;    /* samples of the call                                    */
    int32_t count;   /* frames of the call; -1: over the stride                */
    int32_t restart; /* the state restarts after the call (flush, overflow)    */
    int32_t pad_;
};

/* Constant tables of the transform (built on the host in double, rounded to
 * float) and the handle's mel filterbank as per-filter ranges plus weights:
 * filter j sums wts[off[j] + i] * P[first[j] + i], i = 0 .. len[j] - 1. */
struct FtTab {
    float win[MP3D_FT_WIN];          /* periodic Hann                           */
    float w200[MP3D_FT_HALF][2];     /* exp(-2 pi i m / 200)                    */
    float w400[MP3D_FT_BINS][2];     /* exp(-2 pi i k / 400), k = 0 .. 200      */
    int32_t first[MP3D_FT_MAX_MELS];
    int32_t len[MP3D_FT_MAX_MELS];
    int32_t off[MP3D_FT_MAX_MELS];
    float wts[MP3D_FT_MAX_WTS];
    int32_t n_mels;
    int32_t log10;                   /* MP3D_FEAT_LOG10 set                     */
};

#endif
