/*
 * mp3d_tp_chain.h -- the oversampler's FMA chain, shared by the true-peak tap
 * (mp3d_normalize.hip) and the limiter's detector (mp3d_limiter.hip), device
 * code only (include/mp3d.h "true peak and gain").
 *
 * Oversampled value 4n + p of a channel is u = sum_j taps[p][j] x[n - 5 + j],
 * ONE float32 FMA chain in ascending j from 0.  Both kernels keep a span of
 * sample frames in LDS in runs of MP3D_TP_SEG frames at a stride of
 * MP3D_TP_PAD, a thread slides a register window over one run and its
 * neighbour, and the three non-trivial phases of an index are tp_chain3 on
 * that window: the same operations in the same order, so the detector's
 * values are the tap's bit for bit.
 */
#ifndef MP3D_TP_CHAIN_H
#define MP3D_TP_CHAIN_H

#include "mp3d_normalize.h"

namespace mp3d {

typedef float f32x2 __attribute__((ext_vector_type(2)));

/* One sample frame (all its channels) as the unit of the filter: a float, or
 * a pair whose halves go through the same operations side by side. */
template <int C> struct TpFrame;
template <> struct TpFrame<1> {
    typedef float T;
    static __device__ __forceinline__ T bc(float c) { return c; }
    static __device__ __forceinline__ T fma(T a, T b, T c) { return fmaf(a, b, c); }
    static __device__ __forceinline__ float amax(T v) { return fabsf(v); }
};
template <> struct TpFrame<2> {
    typedef f32x2 T;
    static __device__ __forceinline__ T bc(float c) { return (f32x2){c, c}; }
    static __device__ __forceinline__ T fma(T a, T b, T c) { return __builtin_elementwise_fma(a, b, c); }
    static __device__ __forceinline__ float amax(T v) { return fmaxf(fabsf(v.x), fabsf(v.y)); }
};

/* element e of a span's interleaved samples to its frame's place in the padded runs */
template <int C> __device__ __forceinline__ void tp_put(float *sx, int e, float v) {
    const int j = e / C, c = e - j * C;
    sx[((j >> 4) * MP3D_TP_PAD + (j & 15)) * C + c] = v;
}

/* phases 1..3 of the filter from the device table taps[4][12] into registers */
__device__ __forceinline__ void tp_load_taps(const float *__restrict__ taps, float (&tp)[MP3D_TP_R - 1][MP3D_TP_TAPS]) {
#pragma unroll
    for (int p = 1; p < MP3D_TP_R; p++)
#pragma unroll
        for (int j = 0; j < MP3D_TP_TAPS; j++) tp[p - 1][j] = taps[p * MP3D_TP_TAPS + j];
}

/* a run's frames [0, SEG + HIST) from its place in the padded span (frames
 * from lim on are zeros) */
template <int C>
__device__ __forceinline__ void tp_window(const typename TpFrame<C>::T *p, int lim,
                                          typename TpFrame<C>::T (&w)[MP3D_TP_SEG + MP3D_TP_HIST]) {
#pragma unroll
    for (int k = 0; k < MP3D_TP_SEG + MP3D_TP_HIST; k++)
        w[k] = k < lim ? p[(k / MP3D_TP_SEG) * MP3D_TP_PAD + k % MP3D_TP_SEG] : TpFrame<C>::bc(0.0f);
}

/* the largest |u| of the four phases and all channels of the index whose
 * window starts at w (w[PRE] is the index's own frame: phase 0) */
template <int C>
__device__ __forceinline__ float tp_chain3(const typename TpFrame<C>::T *w,
                                           const float (&tp)[MP3D_TP_R - 1][MP3D_TP_TAPS]) {
    typedef TpFrame<C> Fr;
    typename Fr::T a1 = Fr::bc(0.0f), a2 = Fr::bc(0.0f), a3 = Fr::bc(0.0f);
#pragma unroll
    for (int j = 0; j < MP3D_TP_TAPS; j++) {
        a1 = Fr::fma(Fr::bc(tp[0][j]), w[j], a1);
        a2 = Fr::fma(Fr::bc(tp[1][j]), w[j], a2);
        a3 = Fr::fma(Fr::bc(tp[2][j]), w[j], a3);
    }
    return fmaxf(fmaxf(Fr::amax(w[MP3D_TP_PRE]), Fr::amax(a1)), fmaxf(Fr::amax(a2), Fr::amax(a3)));
}

} // namespace mp3d

#endif
