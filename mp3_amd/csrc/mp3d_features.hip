/*
 * mp3d_features.hip -- the log-mel feature sink: 25 ms periodic-Hann frames
 * every 10 ms of a stream's 16 kHz mono samples, power spectrum, Slaney mel
 * filterbank, optional log10 (include/mp3d.h "log-mel feature sink";
 * DESIGN.md section 4d).
 *
 * Frame t covers x[160 t - 200 .. 160 t + 200), zeros outside the stream.
 * Its 400 windowed real samples y are packed as 200 complex points
 * z[n] = y[2n] + i y[2n + 1]; a 200-point complex FFT (200 = 5 * 5 * 8, three
 * Stockham passes in LDS, every pass storing lane-consecutive points) gives
 * Z, and
 *   X[k] = E[k] + exp(-2 pi i k / 400) O[k],  k = 0 .. 200,
 *   E[k] = (Z[k] + conj Z[200 - k]) / 2,  O[k] = (Z[k] - conj Z[200 - k]) / 2i
 * is the 400-point spectrum of y.  P[k] = |X[k]|^2; filter j sums its
 * weights times P over its bin range in ascending k, one float32 FMA chain.
 *
 * Every frame runs the same sequence of float32 operations whatever call,
 * tile or slot of a tile computes it: samples before the stream start, and
 * after its end in a flushed call, are staged as zeros, and each butterfly,
 * unpack and filter sum is one instance of the same code.
 *
 * Mapping (k_ft_transform): one 256-thread block per (stream, tile of 16
 * frames).  The block stages the tile's span of 16 * 160 + 240 samples --
 * carry, the call's samples, zeros -- and every table (window, twiddles,
 * filter ranges and weights) into LDS; work items (frame, butterfly) of each
 * pass, then (frame, bin) and (frame, filter), are dealt to the threads in
 * order, so consecutive lanes read consecutive points.
 */
#include "mp3d_device.h"
#include "mp3d_features.h"
#include "mp3d_launch.h"

/* A frame's bits may not depend on which copy of a loop body the compiler
 * runs it in (peeled, unrolled, remainder): no implicit contraction, every
 * fused multiply-add below is written as fmaf. */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_FT_MAX_MELS <= MP3D_FT_THREADS, "one thread stages one filter's range");

/* frames emitted once n samples were seen: those with 160 t + 199 <= n - 1 */
__device__ __forceinline__ long long ft_emitted(long long n) {
    return n >= MP3D_FT_HALF ? (n - MP3D_FT_HALF) / MP3D_FT_HOP + 1 : 0;
}
/* first sample the carry holds when frame t is the next to emit */
__device__ __forceinline__ long long ft_carry_base(long long t) {
    const long long a = t * MP3D_FT_HOP - MP3D_FT_HALF;
    return a > 0 ? a : 0;
}

__global__ void __launch_bounds__(MP3D_FT_THREADS)
k_ft_plan(const FtState *__restrict__ st, const int32_t *__restrict__ counts, FtPlan *__restrict__ plan,
          int32_t *__restrict__ feat_count, int n, long long sample_stride, long long feat_stride, int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_FT_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    FtPlan P;
    P.n0 = st[s].n;
    P.t0 = ft_emitted(P.n0);
    P.n_in = (int)c;
    P.restart = flush;
    P.pad_ = 0;
    const long long n1 = P.n0 + c;
    const long long t1 = flush ? (n1 + MP3D_FT_HOP - 1) / MP3D_FT_HOP : ft_emitted(n1);
    const long long k = t1 - P.t0;
    if (k > feat_stride) {
        P.count = -1;
        P.restart = 1;
    } else {
        P.count = (int)k;
    }
    plan[s] = P;
    feat_count[s] = P.count;
}

struct cpx {
    float x, y;
};
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cpx cmul(cpx a, cpx b) {
    return {fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)};
}
__device__ __forceinline__ cpx cmuli_neg(cpx a) { return {a.y, -a.x}; } /* -i a */

/* 4-point DFT of a0 .. a3, forward sign */
__device__ __forceinline__ void dft4(cpx a0, cpx a1, cpx a2, cpx a3, cpx *y) {
    const cpx s0 = cadd(a0, a2), s1 = csub(a0, a2), s2 = cadd(a1, a3), s3 = cmuli_neg(csub(a1, a3));
    y[0] = cadd(s0, s2);
    y[1] = cadd(s1, s3);
    y[2] = csub(s0, s2);
    y[3] = csub(s1, s3);
}

/* 8-point DFT in place, forward sign: the even and the odd points' 4-point
 * transforms, joined by the eighth roots of unity */
__device__ __forceinline__ void dft8(cpx *v) {
    const float h = 0.70710678118654752440f;
    cpx e[4], o[4];
    dft4(v[0], v[2], v[4], v[6], e);
    dft4(v[1], v[3], v[5], v[7], o);
    const cpx o1 = {(o[1].x + o[1].y) * h, (o[1].y - o[1].x) * h}; /* (1 - i) / sqrt 2 */
    const cpx o2 = cmuli_neg(o[2]);
    const cpx o3 = {(o[3].y - o[3].x) * h, (-o[3].x - o[3].y) * h}; /* (-1 - i) / sqrt 2 */
    v[0] = cadd(e[0], o[0]);
    v[4] = csub(e[0], o[0]);
    v[1] = cadd(e[1], o1);
    v[5] = csub(e[1], o1);
    v[2] = cadd(e[2], o2);
    v[6] = csub(e[2], o2);
    v[3] = cadd(e[3], o3);
    v[7] = csub(e[3], o3);
}

/* 5-point DFT in place, forward sign */
__device__ __forceinline__ void dft5(cpx *v) {
    const float C1 = 0.30901699437494742410f, C2 = -0.80901699437494742410f; /* cos 2 pi / 5, cos 4 pi / 5 */
    const float S1 = 0.95105651629515357212f, S2 = 0.58778525229247312917f;  /* sin 2 pi / 5, sin 4 pi / 5 */
    const cpx a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]), b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
    const cpx c1 = {fmaf(C2, a2.x, fmaf(C1, a1.x, v[0].x)), fmaf(C2, a2.y, fmaf(C1, a1.y, v[0].y))};
    const cpx c2 = {fmaf(C1, a2.x, fmaf(C2, a1.x, v[0].x)), fmaf(C1, a2.y, fmaf(C2, a1.y, v[0].y))};
    const cpx d1 = cmuli_neg({fmaf(S2, b2.x, S1 * b1.x), fmaf(S2, b2.y, S1 * b1.y)});
    const cpx d2 = cmuli_neg({fmaf(-S1, b2.x, S2 * b1.x), fmaf(-S1, b2.y, S2 * b1.y)});
    v[0] = cadd(v[0], cadd(a1, a2));
    v[1] = cadd(c1, d1);
    v[4] = csub(c1, d1);
    v[2] = cadd(c2, d2);
    v[3] = csub(c2, d2);
}

/* One radix-5 Stockham pass of every frame of the tile: NS points per
 * sub-transform before the pass, twiddles exp(-2 pi i r k / (5 NS)) from the
 * 200-entry table in steps of 200 / (5 NS). */
template <int NS>
__device__ __forceinline__ void ft_pass5(const cpx *__restrict__ in, cpx *__restrict__ out, const cpx *__restrict__ w200,
                                         int nf, int t) {
    constexpr int Q = MP3D_FT_HALF / 5, STEP = MP3D_FT_HALF / (5 * NS);
    for (int i = t; i < nf * Q; i += MP3D_FT_THREADS) {
        const int f = i / Q, j = i - f * Q, k = j % NS;
        const cpx *src = in + f * MP3D_FT_HALF + j;
        cpx v[5];
        v[0] = src[0];
#pragma unroll
        for (int r = 1; r < 5; r++) v[r] = cmul(src[r * Q], w200[r * k * STEP]);
        dft5(v);
        cpx *dst = out + f * MP3D_FT_HALF + (j - k) * 5 + k;
#pragma unroll
        for (int r = 0; r < 5; r++) dst[r * NS] = v[r];
    }
}

/* The first pass, radix 5 without twiddles: z[n] = (w x)[2n] + i (w x)[2n + 1]
 * read straight from the tile's span sx, points j + 40 r of every frame. */
__device__ __forceinline__ void ft_pass_first(const float *__restrict__ sx, const float *__restrict__ swin,
                                              cpx *__restrict__ out, int nf, int t) {
    constexpr int Q = MP3D_FT_HALF / 5;
    for (int i = t; i < nf * Q; i += MP3D_FT_THREADS) {
        const int f = i / Q, j = i - f * Q;
        const float *x = sx + f * MP3D_FT_HOP;
        cpx v[5];
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const int m = 2 * (j + r * Q);
            const float2 xs = *(const float2 *)(x + m), ws = *(const float2 *)(swin + m);
            v[r] = {xs.x * ws.x, xs.y * ws.y};
        }
        dft5(v);
        cpx *dst = out + f * MP3D_FT_HALF + j * 5;
#pragma unroll
        for (int r = 0; r < 5; r++) dst[r] = v[r];
    }
}

/* The last pass, radix 8 over sub-transforms of 25 points: butterfly j reads
 * and writes points j + 25 r, twiddles exp(-2 pi i r j / 200). */
__device__ __forceinline__ void ft_pass_last(const cpx *__restrict__ in, cpx *__restrict__ out,
                                             const cpx *__restrict__ w200, int nf, int t) {
    constexpr int Q = MP3D_FT_HALF / 8;
    for (int i = t; i < nf * Q; i += MP3D_FT_THREADS) {
        const int f = i / Q, j = i - f * Q;
        const cpx *src = in + f * MP3D_FT_HALF + j;
        cpx v[8];
        v[0] = src[0];
#pragma unroll
        for (int r = 1; r < 8; r++) v[r] = cmul(src[r * Q], w200[r * j]);
        dft8(v);
        cpx *dst = out + f * MP3D_FT_HALF + j;
#pragma unroll
        for (int r = 0; r < 8; r++) dst[r * Q] = v[r];
    }
}

__global__ void __launch_bounds__(MP3D_FT_THREADS)
k_ft_transform(const float *__restrict__ samples, const FtState *__restrict__ st, const FtPlan *__restrict__ plan,
               const FtTab *__restrict__ tab, float *__restrict__ feat, long long sample_stride, long long feat_stride,
               int tiles) {
    __shared__ __attribute__((aligned(16))) float sx[MP3D_FT_SPAN];
    __shared__ __attribute__((aligned(16))) cpx za[MP3D_FT_TILE * MP3D_FT_HALF];
    __shared__ __attribute__((aligned(16))) cpx zb[MP3D_FT_TILE * MP3D_FT_HALF];
    __shared__ __attribute__((aligned(16))) float swin[MP3D_FT_WIN];
    __shared__ __attribute__((aligned(16))) cpx sw200[MP3D_FT_HALF];
    __shared__ __attribute__((aligned(16))) cpx sw400[MP3D_FT_BINS];
    __shared__ __attribute__((aligned(16))) float swts[MP3D_FT_MAX_WTS];
    __shared__ int sfirst[MP3D_FT_MAX_MELS], slen[MP3D_FT_MAX_MELS], soff[MP3D_FT_MAX_MELS];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const FtPlan P = plan[s];
    const int fA = tile * MP3D_FT_TILE;
    if (fA >= P.count) return; /* (also count = -1) */
    const int nf = min(MP3D_FT_TILE, P.count - fA);

    /* tables */
    for (int i = t; i < MP3D_FT_WIN; i += MP3D_FT_THREADS) swin[i] = tab->win[i];
    for (int i = t; i < MP3D_FT_HALF; i += MP3D_FT_THREADS) sw200[i] = {tab->w200[i][0], tab->w200[i][1]};
    for (int i = t; i < MP3D_FT_BINS; i += MP3D_FT_THREADS) sw400[i] = {tab->w400[i][0], tab->w400[i][1]};
    for (int i = t; i < MP3D_FT_MAX_WTS; i += MP3D_FT_THREADS) swts[i] = tab->wts[i];
    if (t < MP3D_FT_MAX_MELS) {
        sfirst[t] = tab->first[t];
        slen[t] = tab->len[t];
        soff[t] = tab->off[t];
    }

    /* the tile's span: sample g0 + i of the stream, from the carry, the
     * call's samples, or zero (before the stream, after a flushed end) */
    const long long g0 = (P.t0 + fA) * MP3D_FT_HOP - MP3D_FT_HALF;
    const long long cb = ft_carry_base(P.t0), n1 = P.n0 + P.n_in;
    const float *carry = st[s].carry;
    const float *row = samples + (size_t)s * (size_t)sample_stride;
    const int span = nf * MP3D_FT_HOP + MP3D_FT_WIN - MP3D_FT_HOP;
    for (int i = t; i < span; i += MP3D_FT_THREADS) {
        const long long g = g0 + i;
        float v = 0.0f;
        if (g >= cb && g < P.n0) v = carry[g - cb];
        else if (g >= P.n0 && g < n1) v = row[g - P.n0];
        sx[i] = v;
    }
    __syncthreads();

    ft_pass_first(sx, swin, zb, nf, t);
    __syncthreads();
    ft_pass5<5>(zb, za, sw200, nf, t);
    __syncthreads();
    ft_pass_last(za, zb, sw200, nf, t);
    __syncthreads();

    /* unpack to the 400-point spectrum's bins 0 .. 200 and their power */
    float *pw = (float *)za; /* [frame][201] */
    for (int i = t; i < nf * MP3D_FT_BINS; i += MP3D_FT_THREADS) {
        const int f = i / MP3D_FT_BINS, k = i - f * MP3D_FT_BINS;
        const cpx *Z = zb + f * MP3D_FT_HALF;
        const cpx a = Z[k == MP3D_FT_HALF ? 0 : k], b = Z[k == 0 ? 0 : MP3D_FT_HALF - k];
        const cpx e = {0.5f * (a.x + b.x), 0.5f * (a.y - b.y)};
        const cpx o = {0.5f * (a.y + b.y), 0.5f * (b.x - a.x)}; /* (a - conj b) / 2i */
        const cpx x = cadd(e, cmul(o, sw400[k]));
        pw[i] = fmaf(x.x, x.x, x.y * x.y);
    }
    __syncthreads();

    /* mel sums, ascending k; (frame, filter) in output order */
    const int nm = tab->n_mels, lg = tab->log10;
    float *out = feat + ((size_t)s * (size_t)feat_stride + (size_t)fA) * (size_t)nm;
    for (int i = t; i < nf * nm; i += MP3D_FT_THREADS) {
        const int f = i / nm, j = i - f * nm;
        const float *p = pw + f * MP3D_FT_BINS + sfirst[j];
        const float *w = swts + soff[j];
        const int len = slen[j];
        float acc = 0.0f;
        for (int q = 0; q < len; q++) acc = fmaf(w[q], p[q], acc);
        out[i] = lg ? log10f(fmaxf(acc, 1e-10f)) : acc;
    }
}

/* the state after the call: the samples from the next frame's start on */
__global__ void __launch_bounds__(MP3D_FT_THREADS)
k_ft_update(const float *__restrict__ samples, FtState *__restrict__ st, const FtPlan *__restrict__ plan,
            long long sample_stride) {
    __shared__ float nc[MP3D_FT_WIN];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x;
    const FtPlan P = plan[s];
    FtState *S = st + s;
    if (P.restart) {
        for (int i = t; i < MP3D_FT_WIN; i += MP3D_FT_THREADS) S->carry[i] = 0.0f;
        if (t == 0) S->n = 0;
        return;
    }
    if (!P.n_in) return;
    const long long n1 = P.n0 + P.n_in;
    const long long cb0 = ft_carry_base(P.t0), cb1 = ft_carry_base(ft_emitted(n1));
    const int keep = (int)(n1 - cb1); /* <= 399 */
    const float *row = samples + (size_t)s * (size_t)sample_stride;
    for (int i = t; i < MP3D_FT_WIN; i += MP3D_FT_THREADS) {
        const long long g = cb1 + i;
        float v = 0.0f;
        if (i < keep) v = g < P.n0 ? S->carry[g - cb0] : row[g - P.n0];
        nc[i] = v;
    }
    __syncthreads();
    for (int i = t; i < MP3D_FT_WIN; i += MP3D_FT_THREADS) S->carry[i] = nc[i];
    if (t == 0) S->n = n1;
}

void launch_features(const float *samples, const int32_t *counts, FtState *st, FtPlan *plan, const FtTab *tab, float *feat,
                     int32_t *feat_count, int n, long long sample_stride, long long feat_stride, int tiles, int flush,
                     hipStream_t strm) {
    const dim3 blk(MP3D_FT_THREADS);
    hipLaunchKernelGGL(k_ft_plan, dim3((n + MP3D_FT_THREADS - 1) / MP3D_FT_THREADS), blk, 0, strm, st, counts, plan,
                       feat_count, n, sample_stride, feat_stride, flush);
    hipLaunchKernelGGL(k_ft_transform, dim3((unsigned)n * (unsigned)tiles), blk, 0, strm, samples, st, plan, tab, feat,
                       sample_stride, feat_stride, tiles);
    hipLaunchKernelGGL(k_ft_update, dim3(n), blk, 0, strm, samples, st, plan, sample_stride);
}

} // namespace mp3d
