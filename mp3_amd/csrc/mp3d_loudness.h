/*
 * mp3d_loudness.h -- data layout of the loudness sink, shared by
 * mp3d_loudness.hip and the host library (include/mp3d.h "loudness sink";
 * DESIGN.md section 4e).
 *
 * A loudness call has a stream's new float32 samples (1 or 2 channels,
 * interleaved) contiguous in device memory and runs five kernels on them:
 *   k_ld_plan    thread / stream : samples before, clamped count, first block,
 *                block count or -1, tile count
 *   k_ld_local   block / (stream, tile) : every thread filters its SEG samples
 *                from a zero state, an affine scan over the lanes of each wave
 *                and a walk over the waves' totals give the tile's end state
 *                from a zero start (z_TILE)
 *   k_ld_carry   wave / stream   : s_{t+1} = A^TILE s_t + z_t over the tiles from
 *                the slot's LdState, 64 tiles per affine scan over the lanes:
 *                every tile's entry state
 *   k_ld_energy  block / (stream, tile) : the scan again, each thread's true
 *                entry state, the filter again, y^2 into the (at most two)
 *                100 ms blocks of the segment, fixed-order reduction to
 *                per-(tile, block) partial sums; the tile's peak
 *   k_ld_finish  block / stream  : partials summed in tile order, z as float32,
 *                count, peak, the new LdState
 * and k_ld_gate (wave / row) is the gated integrated loudness of block rows.
 *
 * The K-weighting cascade (two biquads, transposed direct form II, double) is
 * linear in its 4-vector of state: over g samples s_end = A^g s_start + z_g,
 * z_g the end state from a zero start.  A is the same for both channels.
 */
#ifndef MP3D_LOUDNESS_H
#define MP3D_LOUDNESS_H

#include <stdint.h>

#define MP3D_LD_THREADS 256
#define MP3D_LD_SEG 16                                /* samples one thread filters        */
#define MP3D_LD_TILE 4096                             /* samples one block filters: THREADS * SEG */
#define MP3D_LD_MIN_H 800                             /* the shortest 100 ms block (8 kHz) */
/* the most 100 ms blocks one tile's samples lie in */
#define MP3D_LD_TILE_BLOCKS (MP3D_LD_TILE / MP3D_LD_MIN_H + 2)
/* a thread's samples in LDS: an odd stride, so 64 lanes hit 64 banks */
#define MP3D_LD_PAD (MP3D_LD_SEG + 1)

/* Per-stream loudness state (one per stream slot of the handle, only while
 * loudness is set; NOT part of the StreamState blob).  All zero = restarted. */
struct LdState {
    int64_t n;       /* samples since the restart                               */
    double f[2][4];  /* per channel: stage 1's s1, s2, stage 2's s1, s2          */
    double part;     /* sum of y^2 over the channels of the open block so far    */
};

/* Per-stream plan of one call (k_ld_plan -> the other kernels). */
struct LdPlan {
    int64_t n0;      /* samples seen before the call                            */
    int32_t n_in;    /* samples of the call                                     */
    int32_t count;   /* complete blocks of the call; -1: over the stride        */
    int32_t restart; /* the state restarts after the call (flush, overflow)     */
    int32_t tiles;   /* ceil(n_in / MP3D_LD_TILE)                               */
};

/* Constants of one output rate, built on the host in (long) double. */
struct LdTab {
    double coef[10];                        /* b0 b1 b2 a1 a2 of stage 1, stage 2 */
    double apow[65][16];                    /* A^(SEG t), row-major 4 x 4: the scan over a wave's lanes */
    double tpow[65][16];                    /* A^(TILE t): k_ld_carry's scan over 64 tiles */
    int32_t H;                              /* samples per 100 ms block           */
    int32_t ch;                             /* channels of the packed format      */
};

#endif
