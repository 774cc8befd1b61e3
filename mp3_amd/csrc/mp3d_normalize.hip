/*
 * mp3d_normalize.hip -- the true-peak tap and the gain kernels: a 4x
 * oversampled peak of packed float32 samples, the normalisation gain from
 * loudness and true peak, and a per-stream gain applied to packed PCM
 * (include/mp3d.h "true peak and gain"; DESIGN.md section 4f;
 * mp3d_normalize.h has the kernel list and the layouts).
 *
 * Oversampled value 4n + p of a channel is u = sum_j taps[p][j] x[n - 5 + j],
 * ONE float32 FMA chain in ascending j from 0, whatever call, tile or thread
 * computes it; samples before the stream's start, and after its end in a
 * flushed call, are staged as zeros so the chain has the same length
 * everywhere.  Phase 0 is the delta, so its value is taken as |x[n]|.  The
 * result of a call is a maximum, which is exact: no order of the reduction
 * changes its bits, and a stream fed in other pieces has the same maximum
 * over its calls bit for bit.
 *
 * Mapping (k_tp_peak): one 256-thread block per (stream, tile of 4096 emitted
 * indices).  The block stages the tile's 4096 + 11 sample frames into LDS as
 * they are (a stereo frame's two channels side by side), in runs of 16 frames
 * at a stride of 17.  A thread owns 16 consecutive indices: it reads its
 * 16 + 11 frames into registers once (lane l reads frame 17 l + k: one 4-byte
 * word of 32 banks for mono, one 8-byte pair of 64 banks for stereo, no two
 * lanes of a group on one bank) and slides the three 12-tap chains over them:
 * 16 x 3 x 12 FMAs per channel for 27 LDS reads.  A stereo frame's two chains
 * run as one packed FMA (v_pk_fma_f32: the same IEEE fma in each half), which
 * halves the instruction count of the kernel's bound, the vector ALU.
 */
#include "mp3d_device.h"
#include "mp3d_normalize.h"
#include "mp3d_tp_chain.h"
#include "mp3d_launch.h"

/* the wglds build and the product build must round alike: no implicit
 * contraction, every fused multiply-add below is written as fmaf */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_TP_TILE == MP3D_TP_THREADS * MP3D_TP_SEG, "one segment per thread");
static_assert(MP3D_TP_SEG == 16, "a sample's run and place in it are a shift and a mask");
static_assert(MP3D_TP_PRE + MP3D_TP_POST + 1 == MP3D_TP_TAPS && MP3D_TP_HIST == MP3D_TP_PRE + MP3D_TP_POST,
              "index n reads x[n - PRE .. n + POST]");
static_assert(MP3D_TP_THREADS == 256, "four waves: their maxima are joined by name");
static_assert(2 * MP3D_TP_HIST <= 64 && 2 * MP3D_TP_POST <= MP3D_TP_THREADS, "one thread per history / tail element");
#define MP3D_TP_WAVES (MP3D_TP_THREADS / 64)

__global__ void __launch_bounds__(MP3D_TP_THREADS)
k_tp_plan(const TpState *__restrict__ st, const int32_t *__restrict__ counts, TpPlan *__restrict__ plan, int n,
          long long sample_stride, int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_TP_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    TpPlan P;
    P.n0 = st[s].n;
    P.n_in = (int)c;
    /* index i is emitted once sample i + POST was seen; a flush emits the rest */
    const long long n1 = P.n0 + c;
    const long long e1 = flush ? n1 : n1 > MP3D_TP_POST ? n1 - MP3D_TP_POST : 0;
    P.e0 = P.n0 > MP3D_TP_POST ? P.n0 - MP3D_TP_POST : 0;
    P.n_emit = (int)(e1 - P.e0);
    P.tiles = (P.n_emit + MP3D_TP_TILE - 1) / MP3D_TP_TILE;
    P.restart = flush;
    plan[s] = P;
}

/* A tile's span into LDS: `span` samples from sample i0 of the call (i0 >=
 * -HIST; row: the call's first element).  Samples before the call come from
 * the slot's history, samples past the call's n_in (a flushed end, at most
 * POST of them) are zeros, the rest is loaded 16 bytes at a time from the
 * first aligned element on. */
template <int C>
__device__ __forceinline__ void tp_stage(const float *__restrict__ row, long long i0, int span, int n_in,
                                         const TpState *__restrict__ S, float *sx, int t) {
    const int E = span * C;
    /* elements [elo, ehi) of the span are the call's own */
    const int elo = (int)min((long long)E, (i0 < 0 ? -i0 : 0LL) * C);
    const int ehi = (int)max((long long)elo, min((long long)E, ((long long)n_in - i0) * C));
    if (t < elo) {
        const int j = t / C, c = t - j * C;
        tp_put<C>(sx, t, S->hist[c][MP3D_TP_HIST + (int)i0 + j]);
    }
    if (t < E - ehi) tp_put<C>(sx, ehi + t, 0.0f);
    const int ne = ehi - elo;
    if (ne <= 0) return;
    const float *g = row + (i0 * C + elo);
    const int head = min(ne, (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u));
    if (t < head) tp_put<C>(sx, elo + t, g[t]);
    const int n4 = (ne - head) & ~3;
    for (int k = head + t * 4; k < head + n4; k += MP3D_TP_THREADS * 4) {
        const float4 v = *(const float4 *)(g + k);
        tp_put<C>(sx, elo + k, v.x);
        tp_put<C>(sx, elo + k + 1, v.y);
        tp_put<C>(sx, elo + k + 2, v.z);
        tp_put<C>(sx, elo + k + 3, v.w);
    }
    if (head + n4 + t < ne) tp_put<C>(sx, elo + head + n4 + t, g[head + n4 + t]);
}

/* the largest |u| of one tile's emitted indices, all phases and channels */
template <int C>
__global__ void __launch_bounds__(MP3D_TP_THREADS)
k_tp_peak(const float *__restrict__ samples, const TpState *__restrict__ st, const TpPlan *__restrict__ plan,
          const float *__restrict__ taps, float *__restrict__ tilepk, long long sample_stride, int tiles) {
    __shared__ __attribute__((aligned(16))) float sx[MP3D_TP_RUNS * MP3D_TP_PAD * C];
    __shared__ float pks[MP3D_TP_WAVES];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const TpPlan P = plan[s];
    if (tile >= P.tiles) return;
    const int m = min(MP3D_TP_TILE, P.n_emit - tile * MP3D_TP_TILE);
    /* the span's first sample, counted from the call's first */
    const long long i0 = P.e0 + (long long)tile * MP3D_TP_TILE - MP3D_TP_PRE - P.n0;
    tp_stage<C>(samples + (size_t)s * (size_t)sample_stride * C, i0, m + MP3D_TP_HIST, P.n_in, st + s, sx, t);
    __syncthreads();

    float tp[MP3D_TP_R - 1][MP3D_TP_TAPS]; /* (phase 0 is the delta) */
    tp_load_taps(taps, tp);

    /* this thread's indices: span frames [t SEG, t SEG + cnt + HIST) */
    typedef TpFrame<C> Fr;
    typedef typename Fr::T T;
    const int cnt = max(0, min(MP3D_TP_SEG, m - t * MP3D_TP_SEG));
    const int lim = cnt ? cnt + MP3D_TP_HIST : 0;
    const T *p = (const T *)sx + t * MP3D_TP_PAD;
    T w[MP3D_TP_SEG + MP3D_TP_HIST];
    tp_window<C>(p, lim, w);
    float pk = 0.0f;
#pragma unroll
    for (int i = 0; i < MP3D_TP_SEG; i++) {
        const float v = tp_chain3<C>(w + i, tp); /* (mp3d_tp_chain.h: shared with the limiter's detector) */
        pk = i < cnt ? fmaxf(pk, v) : pk;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d)); /* (a maximum: any order) */
    if ((t & 63) == 0) pks[t >> 6] = pk;
    __syncthreads();
    if (t == 0) tilepk[(size_t)s * tiles + tile] = fmaxf(fmaxf(pks[0], pks[1]), fmaxf(pks[2], pks[3]));
}

/* the call's true peak and the state after it */
__global__ void __launch_bounds__(64)
k_tp_finish(const float *__restrict__ samples, TpState *__restrict__ st, const TpPlan *__restrict__ plan,
            const float *__restrict__ tilepk, float *__restrict__ tpeak, long long sample_stride, int ch, int tiles) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x;
    const TpPlan P = plan[s];
    float pk = 0.0f;
    for (int i = t; i < P.tiles; i += 64) pk = fmaxf(pk, tilepk[(size_t)s * tiles + i]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d));
    if (t == 0) tpeak[s] = pk;

    /* the last HIST samples seen: the call's, before them the old history's */
    TpState *S = st + s;
    const int c = t / MP3D_TP_HIST, k = t - c * MP3D_TP_HIST;
    const bool mine = t < ch * MP3D_TP_HIST;
    float h = 0.0f;
    if (mine && !P.restart) {
        const long long i = (long long)P.n_in - MP3D_TP_HIST + k;
        h = i < 0 ? S->hist[c][P.n_in + k] : samples[((size_t)s * (size_t)sample_stride + (size_t)i) * ch + c];
    }
    __syncthreads(); /* every read of the old state is before the new one's stores */
    if (P.restart) {
        if (t < 2 * MP3D_TP_HIST) S->hist[c][k] = 0.0f;
        if (t == 0) S->n = 0;
    } else if (P.n_in) {
        if (mine) S->hist[c][k] = h;
        if (t == 0) S->n = P.n0 + P.n_in;
    }
}

/* g = 10^((target - lufs) / 20), limited so that g * tpeak <= c; 1 for a
 * loudness that is not finite */
__global__ void __launch_bounds__(MP3D_GA_THREADS)
k_gain_calc(const float *__restrict__ lufs, const float *__restrict__ tpeak, float *__restrict__ gain, int n,
            double target, double c) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_GA_THREADS + threadIdx.x;
    if (s >= n) return;
    const float l = lufs[s];
    double g = 1.0;
    if (isfinite(l)) {
        g = pow(10.0, (target - (double)l) / 20.0);
        if (tpeak) {
            const double tp = (double)tpeak[s];
            if (tp > 0.0 && g * tp > c) g = c / tp;
        }
    }
    gain[s] = (float)g;
}

/* V scaled elements from in to out, 16 bytes per store */
template <bool F32> struct GaOut;
template <> struct GaOut<true> {
    typedef float T;
    static constexpr int V = 4;
    static __device__ __forceinline__ T one(float y) { return y; }
    static __device__ __forceinline__ void vec(const float *in, T *out, float g) {
        const float4 a = *(const float4 *)in;
        *(float4 *)out = make_float4(a.x * g, a.y * g, a.z * g, a.w * g);
    }
};
template <> struct GaOut<false> {
    typedef short T;
    static constexpr int V = 8;
    static __device__ __forceinline__ T one(float y) { return pcm_i16(y); }
    static __device__ __forceinline__ unsigned pair(float lo, float hi) {
        return (unsigned)(unsigned short)pcm_i16(lo) | ((unsigned)(unsigned short)pcm_i16(hi) << 16);
    }
    static __device__ __forceinline__ void vec(const float *in, T *out, float g) {
        const float4 a = *(const float4 *)in, b = *(const float4 *)(in + 4);
        *(uint4 *)out = make_uint4(pair(a.x * g, a.y * g), pair(a.z * g, a.w * g), pair(b.x * g, b.y * g),
                                   pair(b.z * g, b.w * g));
    }
};

/* out = samples * gain[s] for the stream's first counts[s] sample frames (C
 * channels each), nothing past them; ccnt[s] is the clamped count.  in and
 * out are not __restrict__: float32 may run in place, every element is read
 * by the thread that writes it, before it does. */
template <int C, bool F32>
__global__ void __launch_bounds__(MP3D_GA_THREADS)
k_gain_apply(const float *samples, const int32_t *__restrict__ counts, const float *__restrict__ gain, void *out,
             int32_t *__restrict__ ccnt, long long sample_stride, int chunks) {
    MP3D_LDS_ENTRY();
    typedef GaOut<F32> O;
    const int s = blockIdx.x / chunks, ck = blockIdx.x % chunks, t = threadIdx.x;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    if (ck == 0 && t == 0) ccnt[s] = (int32_t)c;
    const long long ne = c * C, e0 = (long long)ck * MP3D_GA_CHUNK;
    if (e0 >= ne) return;
    const int m = (int)min((long long)MP3D_GA_CHUNK, ne - e0);
    const float g = gain[s];
    const size_t at = (size_t)s * (size_t)sample_stride * C + (size_t)e0;
    const float *in = samples + at;
    typename O::T *o = (typename O::T *)out + at;
    int done = 0;
    if ((((uintptr_t)in | (uintptr_t)o) & 15) == 0) {
        done = m & ~(O::V - 1);
        for (int e = t * O::V; e < done; e += MP3D_GA_THREADS * O::V) O::vec(in + e, o + e, g);
    }
    for (int e = done + t; e < m; e += MP3D_GA_THREADS) o[e] = O::one(in[e] * g);
}

void launch_true_peak(const float *samples, const int32_t *counts, TpState *st, TpPlan *plan, const float *taps,
                      float *tilepk, float *tpeak, int n, long long sample_stride, int ch, int tiles, int flush,
                      hipStream_t strm) {
    const dim3 blk(MP3D_TP_THREADS), grid((unsigned)n * (unsigned)tiles);
    hipLaunchKernelGGL(k_tp_plan, dim3((n + MP3D_TP_THREADS - 1) / MP3D_TP_THREADS), blk, 0, strm, st, counts, plan, n,
                       sample_stride, flush);
    if (ch == 2)
        hipLaunchKernelGGL(k_tp_peak<2>, grid, blk, 0, strm, samples, st, plan, taps, tilepk, sample_stride, tiles);
    else
        hipLaunchKernelGGL(k_tp_peak<1>, grid, blk, 0, strm, samples, st, plan, taps, tilepk, sample_stride, tiles);
    hipLaunchKernelGGL(k_tp_finish, dim3(n), dim3(64), 0, strm, samples, st, plan, tilepk, tpeak, sample_stride, ch,
                       tiles);
}

void launch_gain_calc(const float *lufs, const float *tpeak, float *gain, int n, double target, double c,
                      hipStream_t strm) {
    hipLaunchKernelGGL(k_gain_calc, dim3((n + MP3D_GA_THREADS - 1) / MP3D_GA_THREADS), dim3(MP3D_GA_THREADS), 0, strm,
                       lufs, tpeak, gain, n, target, c);
}

void launch_gain_apply(const float *samples, const int32_t *counts, const float *gain, void *out, int32_t *ccnt,
                       bool f32, int ch, int n, long long sample_stride, int chunks, hipStream_t strm) {
    const dim3 blk(MP3D_GA_THREADS), grid((unsigned)n * (unsigned)chunks);
    if (ch == 2) {
        if (f32)
            hipLaunchKernelGGL((k_gain_apply<2, true>), grid, blk, 0, strm, samples, counts, gain, out, ccnt,
                               sample_stride, chunks);
        else
            hipLaunchKernelGGL((k_gain_apply<2, false>), grid, blk, 0, strm, samples, counts, gain, out, ccnt,
                               sample_stride, chunks);
    } else {
        if (f32)
            hipLaunchKernelGGL((k_gain_apply<1, true>), grid, blk, 0, strm, samples, counts, gain, out, ccnt,
                               sample_stride, chunks);
        else
            hipLaunchKernelGGL((k_gain_apply<1, false>), grid, blk, 0, strm, samples, counts, gain, out, ccnt,
                               sample_stride, chunks);
    }
}

} // namespace mp3d
