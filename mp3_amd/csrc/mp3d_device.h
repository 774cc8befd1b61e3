/*
 * mp3d_device.h -- device-side definitions shared by the kernels of the
 * batched MP3 decode hot path (mp3d_demux.hip, mp3d_huffman.hip,
 * mp3d_synth.hip; ISO/IEC 11172-3 / 13818-3).
 *
 * Pipeline for one batch call (all on one HIP stream, state resident in HBM):
 *   k_demux    wave   / stream  : header + side-info walk, bit-reservoir map,
 *                                 main-data bytes -> contiguous md region
 *   k_huffman  thread / unit    : scalefactors + Huffman (LDS LUT) -> is[576]
 *   k_synth    wave   / stream  : requantise, stereo, alias, IMDCT, overlap,
 *                                 32-band matrixing + 512-tap window -> PCM
 * A unit is one (frame, granule, channel).  Streams are independent, so the
 * batch is embarrassingly parallel over streams; frames of one stream are
 * walked in order inside k_demux / k_synth, which keep the per-stream state
 * (reservoir, overlap, synthesis FIFO) in registers / LDS between frames.
 * The reference (lxm0851/mp3) has no decoder source: its player's decode
 * loop (REF/README.md:2-3) is the path these kernels replace.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "mp3d_internal.h"
#include "mp3d_tables.h"

namespace mp3d {

struct DevInfo { /* mirrors mp3d_frame_info (include/mp3d.h) */
    int32_t frame_bytes, channels, hz, layer, bitrate_kbps, samples;
};

#define REC_TAG 0x80  /* FrameRec.first_gr high bit: Xing/Info tag frame           */
#define REC_DROP 0x40 /* dropped frame (invalid side info, CRC mismatch)            */

/* One wave per data region: LDS operations of a wave complete in issue
 * order, so an LDS hand-off between lanes of ONE wave only needs the
 * compiler not to reorder across it -- no s_barrier and, unlike
 * __syncthreads(), no vmcnt(0) drain of loads/stores still in flight.    */
__device__ __forceinline__ void wave_sync() { __asm__ volatile("" ::: "memory"); }

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

/* The library's int16 rounding of a float32 sample, wherever packed PCM is
 * stored as int16 (mp3d_resample.hip rs_store, mp3d_normalize.hip
 * k_gain_apply): clamp(floor(y * 32768 + 0.5)) of the exact product
 * (v + 0.5f itself could round up across an integer): the scaling and
 * v - floor(v) are exact */
__device__ __forceinline__ short pcm_i16(float y) {
    const float v = y * 32768.0f, fl = floorf(v);
    const float r = v - fl >= 0.5f ? fl + 1.0f : fl;
    return (short)fminf(fmaxf(r, -32768.0f), 32767.0f);
}

/* MP3D_LDS_ENTRY(): the first statement of every kernel (tests/
 * test_wglds_coverage.py), nothing in the product build.  In the debug build
 * libmp3d_wglds.so (-DMP3D_WG_LDS_POISON, mp3_amd/_build.py) every workgroup
 * fills its whole static LDS allocation [0, group_segment_fixed_size) with
 * 0xFF before anything else, then meets at a barrier: a read of LDS the
 * workgroup itself did not write sees all-ones words (NaN as float) in EVERY
 * workgroup, not what the previous workgroup on the CU left.  The launch-level
 * k_lds_poison only reaches the first workgroup placed on a CU. */
#ifdef MP3D_WG_LDS_POISON
typedef volatile __attribute__((address_space(3))) uint32_t lds_vu32;
typedef volatile __attribute__((address_space(3))) uint8_t lds_vu8;
__device__ __forceinline__ void lds_entry_fill() {
    const uint32_t bytes = __builtin_amdgcn_groupstaticsize();
    const uint32_t nt = blockDim.x * blockDim.y * blockDim.z;
    const uint32_t t = (threadIdx.z * blockDim.y + threadIdx.y) * blockDim.x + threadIdx.x;
    /* static LDS starts at LDS address 0 (an integer made a pointer, not a
     * null pointer constant: that one is ~0 in this address space) */
    for (uint32_t i = t; i < bytes / 4u; i += nt) *(lds_vu32 *)(uintptr_t)(i * 4u) = 0xFFFFFFFFu;
    for (uint32_t i = (bytes & ~3u) + t; i < bytes; i += nt) *(lds_vu8 *)(uintptr_t)i = 0xFFu;
    __syncthreads();
}
#define MP3D_LDS_ENTRY() ::mp3d::lds_entry_fill()
#else
#define MP3D_LDS_ENTRY()
#endif

} // namespace mp3d
