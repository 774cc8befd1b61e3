/*
 * mp3d_limiter.h -- data layout of the look-ahead true-peak limiter, shared by
 * mp3d_limiter.hip and the host library (include/mp3d.h "limiter"; DESIGN.md
 * section 4h).
 *
 * A limiter call has a stream's new float32 samples (1 or 2 channels,
 * interleaved) contiguous in device memory and runs three kernels on them:
 *   k_lim_plan   thread / stream : samples before, clamped count, the first
 *                and last emitted index, the overflow, tile count, restart
 *                flag, out_count[s]
 *   k_lim_tile   block / (stream, tile of MP3D_LIM_TILE emitted indices) : the
 *                tile's frames and a halo of 3A + 5 back and A + 6 ahead into
 *                LDS as v = x * gain (from the slot's carry before the call's
 *                first sample, zeros outside the stream), in the true-peak
 *                tap's padded runs; the tap's three FMA chains and |v| per
 *                index of the halo, R = floor(c / p * 2^20) as int32 into LDS;
 *                the sliding minimum over [k - 2A, k + A] with a thread per
 *                run of 16 minima: the end of its own run, the whole runs in
 *                between from a doubled array of run minima (a word per
 *                thread, six small steps), and a running minimum into the run
 *                where its windows end; a running sum of the minima over the
 *                workgroup (uint32, differences are exact) for
 *                the box of A + 1; y = v * (float)G * 2^-20 stored coalesced
 *                as float32 or int16; the tile's smallest gain
 *   k_lim_carry  block / stream  : the minimum over the tiles into gr[s], the
 *                slot's new carry and sample count
 *
 * LDS of k_lim_tile at two channels: the span is MP3D_LIM_TILE + MP3D_LIM_HALO
 * = 6027 frames in 377 runs of 17 frames (51 272 bytes), the integer array
 * MP3D_LIM_NR = 6144 words in padded runs and one run more (6545 words,
 * 26 180 bytes), two buffers of 416 run minima (3 328 bytes), six wave totals
 * and six wave minima (48 bytes): 80 828 bytes of arrays, which the compiler
 * lays out in 80 856 (28 bytes of alignment padding), two workgroups of six
 * waves per compute unit (160 KB).  One channel: 55 192 bytes of arrays in
 * 55 224.  MP3D_LIM_THREADS x 16 covers TILE + 4 AMAX: the chains of a tile
 * are one round with every thread at work.
 */
#ifndef MP3D_LIMITER_H
#define MP3D_LIMITER_H

#include <stdint.h>
#include "mp3d_normalize.h"

#define MP3D_LIM_THREADS 384
#define MP3D_LIM_TILE 4096                              /* emitted indices one block computes          */
#define MP3D_LIM_AMAX 480                               /* A = (fs + 50) / 100 at 48 kHz               */
#define MP3D_LIM_Q 1048576                              /* gains are integers in units of 2^-20        */
#define MP3D_LIM_BACK(A) (3 * (A) + MP3D_TP_PRE)        /* frames a tile reads before its first index  */
#define MP3D_LIM_AHEAD(A) ((A) + MP3D_TP_POST)          /* ... and after its last: the emit delay      */
#define MP3D_LIM_HALO (MP3D_LIM_BACK(MP3D_LIM_AMAX) + MP3D_LIM_AHEAD(MP3D_LIM_AMAX)) /* 1931 at 48 kHz */
#define MP3D_LIM_CARRY MP3D_LIM_HALO                    /* sample frames of v carried between calls    */
#define MP3D_LIM_SPAN (MP3D_LIM_TILE + MP3D_LIM_HALO)   /* frames of a tile's span                     */
#define MP3D_LIM_RUNS ((MP3D_LIM_SPAN + MP3D_TP_SEG - 1) / MP3D_TP_SEG)
#define MP3D_LIM_RSEG 16                                /* R values per thread: its run                */
#define MP3D_LIM_NR (MP3D_LIM_THREADS * MP3D_LIM_RSEG)  /* >= TILE + 4 AMAX required gains             */
#define MP3D_LIM_PSEG 16                                /* minima per thread in the running sum: one padded run */

/* Per-stream limiter state (one per stream slot of the handle, only while the
 * limiter is set; NOT part of the StreamState blob).  n = 0 is restarted: the
 * carry is then not read. */
struct LimState {
    int64_t n;                         /* samples since the restart                            */
    float carry[MP3D_LIM_CARRY * 2];   /* v[n - (4A + 11) .. n), interleaved by the format's channels */
};

/* Per-stream plan of one call (k_lim_plan -> the other kernels). */
struct LimPlan {
    int64_t n0;      /* samples seen before the call                         */
    int64_t e0;      /* first index the call emits                           */
    int32_t n_in;    /* samples of the call                                  */
    int32_t n_emit;  /* indices the call emits: [e0, e0 + n_emit); 0 on overflow */
    int32_t tiles;   /* ceil(n_emit / MP3D_LIM_TILE)                         */
    int32_t restart; /* the state restarts after the call (flush, overflow)  */
};

#endif
