/*
 * mp3d_stretch.h -- data layout of the tempo sink (WSOLA time stretch),
 * shared by mp3d_stretch.hip and the host library (include/mp3d.h "tempo
 * sink").
 *
 * A stretch call has a stream's new float32 samples (1 or 2 channels,
 * interleaved) contiguous in device memory and runs two kernels on them:
 *   k_st_plan    thread / stream : samples before, clamped count, the blocks
 *                the data-independent emit rule releases (a bisection over
 *                e_k), the output count, the overflow and restart flags
 *   k_st_blocks  block / stream  : the stream's blocks one after the other
 *                (a_k needs a_{k-1}).  Per block: the 11-bit match signal q of
 *                the reference segment and of the candidate span into LDS as
 *                int16, the span in an even-phase and an odd-phase copy so a
 *                candidate of either parity reads aligned pairs; d = E_ref +
 *                E(delta) - 2 X(delta): a thread per two candidates of one
 *                parity sums X two samples per packed int16 dot product, E is
 *                a running sum of the span's squares over the workgroup,
 *                E_ref is the same for all and dropped; the smallest
 *                (d, |delta|, sign) key over the workgroup; the crossfade from
 *                the carry / the call's samples to out; then the new StState.
 */
#ifndef MP3D_STRETCH_H
#define MP3D_STRETCH_H

#include <stdint.h>

#define MP3D_ST_THREADS 256
#define MP3D_ST_HMAX 480                        /* H = (fs + 50) / 100 at 48 kHz            */
#define MP3D_ST_DMAX (MP3D_ST_HMAX / 2)         /* D = H / 2                                */
#define MP3D_ST_SPAN (MP3D_ST_HMAX + 2 * MP3D_ST_DMAX) /* samples any candidate of a block reads */
#define MP3D_ST_QMAX 1023                       /* |q| <= 1023: (2 * 1023)^2 * 480 < 2^31   */
#define MP3D_ST_TEMPO_MAX 4096                  /* 1 <= num, den <= 4096                    */
/* Sample frames carried between calls.  After a call that saw N samples the
 * next block k has N <= e_k, and the carry starts at c = max(0, min(r_k,
 * t_k - D)) with r_k >= t_{k-1} + H - D.  With g = t_k - t_{k-1} in
 * [H/2, 2H] and t_{k+1} - t_k <= 2H:
 *   N <= max(t_k, t_{k-1} + H) + D + H - 1:  N - c <= |g - H| + 2D + H - 1 <= 2H + 2D - 1
 *   N <= t_{k+1} - 1:                        N - c <= 2H + max(D, g - H + D) - 1 <= 3H + D - 1
 * so N - c <= 3H + D - 1 at every tempo. */
#define MP3D_ST_CARRY (3 * MP3D_ST_HMAX + MP3D_ST_DMAX)

/* Per-stream stretch state (one per stream slot of the handle, only while
 * stretch is set; NOT part of the StreamState blob).  All zero = restarted.
 * The slot's tempo is kept apart (it outlives a restart). */
struct StState {
    int64_t n;  /* samples since the restart                               */
    int64_t k;  /* the next block                                          */
    int64_t r;  /* r_k = a_{k-1} + H (0 at k = 0)                          */
    int64_t c0; /* the carry's first sample frame: carry holds [c0, n)     */
    float carry[MP3D_ST_CARRY * 2]; /* interleaved by the format's channels */
};

/* Per-stream plan of one call (k_st_plan -> k_st_blocks). */
struct StPlan {
    int32_t n_in;    /* samples of the call                                  */
    int32_t blocks;  /* blocks the call emits: k .. k + blocks - 1           */
    int32_t n_out;   /* samples the call emits (the last block may be cut);
                        -1: over out_stride, nothing is written              */
    int32_t restart; /* the state restarts after the call (flush, overflow)  */
};

#endif
