/*
 * mp3d_segment.h -- data layout of the segment sink, shared by
 * mp3d_segment.hip and the host library (include/mp3d.h "segment sink";
 * DESIGN.md section 4i).
 *
 * A segment call has a stream's new float32 samples (1 or 2 channels,
 * interleaved) contiguous in device memory and runs three kernels on them:
 *   k_sg_plan    thread / stream : clamped count, the hops the call touches
 *                and completes, tile count
 *   k_sg_energy  block / (stream, tile of MP3D_SG_TILE hops) : a wave per hop
 *                reads the hop's samples of the call with 16-byte loads (a
 *                peel of whole frames up to the first aligned address and
 *                after the last), quantises the mono mix to int16, sums the
 *                squares into uint64 and reduces over the wave; the hop the
 *                call found open starts from the state's partial energy, the
 *                hop it leaves open goes to part[s]; the tile's activity bits
 *                E >= thr as one 64-bit word to bits[s][tile]
 *   k_sg_emit    wave / stream   : chunks of MP3D_SG_CHUNK hops as one 64-bit
 *                word per lane, from the state's history bits and the call's
 *                words; fill and drop are sliding ORs over the whole chunk
 *                (doubling shifts across the lanes), edges are two ANDs; the
 *                segments compacted in order by popcount and a scan over the
 *                lanes; the new state
 *
 * LDS: k_sg_energy holds its four waves' 16 bits each (16 bytes), k_sg_emit
 * the history while it is replaced (128 bytes).
 */
#ifndef MP3D_SEGMENT_H
#define MP3D_SEGMENT_H

#include <stdint.h>

#define MP3D_SG_THREADS 256                 /* k_sg_energy: four waves                         */
#define MP3D_SG_TILE 64                     /* hops one block of k_sg_energy computes: a word  */
#define MP3D_SG_HOPS_PER_WAVE (MP3D_SG_TILE / (MP3D_SG_THREADS / 64))
#define MP3D_SG_MAXHOPS 256                 /* the largest pause and the largest shortest segment, in hops */
#define MP3D_SG_HIST 1024                   /* bits of a kept per slot: 2 (S + P) at S = P = 256 */
#define MP3D_SG_HWORDS (MP3D_SG_HIST / 64)
#define MP3D_SG_CHUNK 4096                  /* hops k_sg_emit holds at a time: a word per lane */
#define MP3D_SG_HMAX 480                    /* H = (fs + 50) / 100 at 48 kHz                   */

/* Per-stream segment state (one per stream slot of the handle, only while the
 * sink is set; NOT part of the StreamState blob).  All zero is restarted. */
struct SgState {
    int64_t n;                      /* samples since the restart                                  */
    uint64_t epart;                 /* energy of the open hop's n % H samples                     */
    int64_t b0;                     /* the last rising edge of o among the decided hops           */
    uint64_t hist[MP3D_SG_HWORDS];  /* a[B - 1024 .. B), bit k of word j is hop B - 1024 + 64 j + k; 0 before hop 0 */
};

/* Per-stream plan of one call (k_sg_plan -> the other kernels). */
struct SgPlan {
    int64_t n0;      /* samples seen before the call                                 */
    int64_t hop0;    /* hops known before the call: n0 / H, the open hop's index     */
    int32_t r0;      /* samples of the open hop seen before the call: n0 % H         */
    int32_t n_in;    /* samples of the call                                          */
    int32_t touched; /* hops the call's samples (or the open hop) lie in             */
    int32_t done;    /* hops the call completes: the first `done` of them            */
    int32_t tiles;   /* ceil(touched / MP3D_SG_TILE)                                 */
    int32_t pad_;
};

#endif
