/*
 * mp3d_pitch.h -- data layout of the pitch sink, shared by mp3d_pitch.hip and
 * the host library (include/mp3d.h "pitch sink").
 *
 * A pitch call has a stream's new float32 samples (1 or 2 channels,
 * interleaved) contiguous in device memory and runs three kernels on them, in
 * this order on the call's stream:
 *   k_pt_plan    thread / stream : clamped count, the samples and frames known
 *                before the call, the frames it emits (or -1), tile count
 *   k_pt_frames  block / (stream, tile of MP3D_PT_TILE frames) : the tile's
 *                samples quantised once into LDS (the carry, then the call's
 *                samples, zeros behind them), then frame by frame the block
 *                floating point shift, the prefix sum of the squares, the
 *                cross sums X(tau) by packed int16 dot products, D, its
 *                running sum S in 64 bits, the two min-reductions and the
 *                record.  It reads the slot's carry and N and writes neither.
 *   k_pt_update  block / stream  : the new carry (the last min(N, SPAN - 1)
 *                quantised samples) and N, or the restart.  It is launched
 *                after k_pt_frames, so no frame reads a carry that the call
 *                itself replaced; inside it the new carry goes through LDS, a
 *                barrier between the last read of the old one and the first
 *                store of the new.
 *
 * The cross sums: thread t of k_pt_frames has parity p = u & 1 and lag group
 * g = u >> 1 (u = t mod the threads that the lag range needs) and owns the
 * four lags 8 g + p + 2 k, k < 4: one parity, a word apart, so a window of
 * eight words of copy p of the frame (copy 1 lies one sample ahead) slides
 * over them, four new words per 16-byte read against four reference words of
 * one broadcast 16-byte read: 16 dot products per two reads.  Where the lag
 * range leaves threads over (T + 1 <= 504), the sample pairs are split among
 * MP3D_PT_THREADS / threads-needed segments and the integer partial sums are
 * added afterwards.  The copies lie 32 banks apart mod 64, which puts the two
 * parities of a 16-lane read group on disjoint banks.
 */
#ifndef MP3D_PITCH_H
#define MP3D_PITCH_H

#include <stdint.h>

#define MP3D_PT_THREADS 256   /* k_pt_frames, k_pt_update: four waves                        */
#define MP3D_PT_TILE 8        /* frames one block of k_pt_frames computes                    */
#define MP3D_PT_HMAX 480      /* H = (fs + 50) / 100 at 48 kHz                               */
#define MP3D_PT_TMAX 961      /* T = floor(fs / fmin) + 1 at 48 kHz and 50 Hz                */
#define MP3D_PT_SPANMAX (2 * MP3D_PT_HMAX + MP3D_PT_TMAX)
#define MP3D_PT_CARRY (MP3D_PT_SPANMAX - 1)
#define MP3D_PT_LAGS 4        /* lags of one parity per thread                               */
#define MP3D_PT_ROW 2112      /* int16 per copy of a frame: 1056 words, 32 mod 64            */
#define MP3D_PT_STAGE ((MP3D_PT_TILE - 1) * MP3D_PT_HMAX + MP3D_PT_SPANMAX)

/* Per-stream pitch state (one per stream slot of the handle, only while the
 * sink is set; NOT part of the StreamState blob).  All zero is restarted. */
struct PtState {
    int64_t n;                     /* samples since the restart                          */
    int16_t carry[MP3D_PT_CARRY + 1]; /* q[n - min(n, SPAN - 1) .. n), from carry[0] on  */
};

/* Per-stream plan of one call (k_pt_plan -> the other kernels). */
struct PtPlan {
    int64_t n0;      /* samples seen before the call                                 */
    int64_t f0;      /* frames known before the call                                 */
    int32_t n_in;    /* samples of the call                                          */
    int32_t emit;    /* frames the call emits; 0 after an overflow                   */
    int32_t tiles;   /* ceil(emit / MP3D_PT_TILE)                                    */
    int32_t restart; /* a flush or an overflow: the slot restarts                    */
};

#endif
