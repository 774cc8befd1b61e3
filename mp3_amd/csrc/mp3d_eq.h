/*
 * mp3d_eq.h -- data layout of the equaliser sink, shared by mp3d_eq.hip and
 * the host library (include/mp3d.h "equaliser sink").
 *
 * An equaliser call has a stream's new float32 samples (1 or 2 channels,
 * interleaved) contiguous in device memory and runs four kernels on them:
 *   k_eq_plan    thread / stream : clamped count, overflow (out_count -1, the
 *                slot restarted), tile count; a slot that restarts without a
 *                sample is zeroed here
 *   k_eq_local   block / (stream, tile), for every tile that another tile
 *                follows (not launched when no stream has two tiles): the
 *                cascade over the tile from a zero state, stage by stage; the
 *                tile's end state z_TILE, a 2K-vector per channel
 *   k_eq_carry   block of K waves / (stream, channel) : s_{t+1} = A^TILE s_t + z_t
 *                with the cascade's full 2K x 2K transition matrix over the
 *                tiles from the slot's EqState, 64 tiles per affine scan over
 *                the lanes, a wave per stage (two rows of every product):
 *                every tile's entry state
 *   k_eq_apply   block / (stream, tile) : the same pass from the tile's true
 *                entry state; float32 out, 16 bytes per store where the row
 *                allows; the thread that holds the call's last sample stores
 *                the slot's new EqState
 *
 * The pass over a tile.  A thread holds its SEG samples of every channel as
 * doubles in registers.  The cascade is block-triangular (stage k's state
 * depends on the stages up to k only), so within a tile it is taken one stage
 * at a time, each a 2-state system of its own: the thread filters its samples
 * from a zero state (z of its segment); an affine scan over the lanes of its
 * wave with the stage's 2 x 2 A_k^(SEG d), in registers, and a walk over the
 * waves' totals through LDS give the stage's state at the thread's first
 * sample; the thread filters again from there and keeps the outputs, which are
 * the next stage's true inputs.  One barrier per stage.
 *
 * LDS of k_eq_local and k_eq_apply at two channels: the samples in padded runs
 * (2 x 256 x 17 floats, 34 816 bytes) and two buffers of wave totals (256
 * bytes); one channel: 17 408 + 128.  k_eq_carry: two buffers of 64 x 21
 * doubles and two entry states, 21 824 bytes.
 */
#ifndef MP3D_EQ_H
#define MP3D_EQ_H

#include <stdint.h>

#define MP3D_EQ_THREADS 256
#define MP3D_EQ_SEG 16                           /* samples one thread filters               */
#define MP3D_EQ_TILE 4096                        /* samples one block filters: THREADS * SEG */
#define MP3D_EQ_PAD (MP3D_EQ_SEG + 1)            /* a thread's samples in LDS: an odd stride */
#define MP3D_EQ_BANDS 10                         /* = MP3D_EQ_MAX_BANDS of include/mp3d.h    */
#define MP3D_EQ_NS (2 * MP3D_EQ_BANDS)           /* state doubles per channel                */
#define MP3D_EQ_TSTRIDE (2 * MP3D_EQ_NS)         /* doubles per (stream, tile) of tz, entry  */

/* Per-stream equaliser state (one per stream slot of the handle, only while
 * the equaliser is set; NOT part of the StreamState blob).  All zero =
 * restarted.  Entries past 2 K stay zero. */
struct EqState {
    double f[2][MP3D_EQ_NS]; /* per channel: stage 1's s1, s2, stage 2's s1, s2, ... */
};

/* Per-stream plan of one call (k_eq_plan -> the other kernels). */
struct EqPlan {
    int32_t n_in;    /* samples of the call; 0 on overflow                     */
    int32_t tiles;   /* ceil(n_in / MP3D_EQ_TILE)                              */
    int32_t restart; /* the state restarts after the call (flush, overflow)    */
    int32_t pad_;
};

/* Constants of one curve at one rate, built on the host in long double.  The
 * cascade's own powers A^(TILE t), t = 0 .. 64, row-major 2K x 2K each, are a
 * buffer of their own (65 (2K)^2 doubles). */
struct EqTab {
    int32_t K;                              /* sections                                   */
    int32_t ch;                             /* channels of the packed format              */
    double coef[5 * MP3D_EQ_BANDS];         /* b0 b1 b2 a1 a2 of stage 1, stage 2, ...    */
    double apow[MP3D_EQ_BANDS][65][4];      /* A_k^(SEG t), row-major 2 x 2               */
};

#endif
