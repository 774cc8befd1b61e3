/*
 * mp3d_eq.hip -- the equaliser sink: a cascade of up to ten caller-designed
 * biquads over the packed output, parallel in time (include/mp3d.h "equaliser
 * sink"; mp3d_eq.h has the kernel list and the layouts).
 *
 * The arithmetic is the loudness sink's (mp3d_loudness.hip): transposed direct
 * form II in double, a run of g samples maps the state affinely, s_end = A^g
 * s_start + z_g, every thread filters MP3D_EQ_SEG samples from a zero state, a
 * log-step scan over the lanes of a wave and a walk over the waves' totals
 * give its true entry state, and it filters again from there.  What differs:
 * the coefficients and the number of sections are the caller's, so inside a
 * tile the cascade is taken stage by stage with 2 x 2 matrices (stage k + 1
 * reads stage k's true outputs from the thread's registers) and only the
 * carry over the tiles uses the cascade's full 2K x 2K matrix; and the result
 * is written back as float32 samples.
 *
 * Everything after the float32 sample is double, rounded once to float32 at
 * the end.  No floating-point atomics and one fixed order for every sum: the
 * same call on the same state gives the same bits.  Tiles are counted from the
 * call's first sample, so a stream fed in other pieces adds in another order:
 * equal within the bound of include/mp3d.h, not bit for bit.
 */
#include "mp3d_device.h"
#include "mp3d_eq.h"
#include "mp3d_launch.h"

/* the wglds build and the product build must round alike: no implicit
 * contraction, every fused multiply-add below is written as fma */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_EQ_TILE == MP3D_EQ_THREADS * MP3D_EQ_SEG, "a thread per segment of the tile");
static_assert(MP3D_EQ_THREADS % 64 == 0 && MP3D_EQ_NS <= 64, "whole waves; a lane per state in k_eq_carry");
#define MP3D_EQ_WAVES (MP3D_EQ_THREADS / 64)

/* one sample through one section: s = {s1, s2}, q = {b0 b1 b2 a1 a2}; the new
 * state is kept only when `keep` (a thread's samples past the call's last) */
template <bool PRED>
__device__ __forceinline__ double eq_step(double v, double *s, const double *q, bool keep) {
    const double o = fma(q[0], v, s[0]);
    const double n1 = fma(q[1], v, fma(-q[3], o, s[1]));
    const double n2 = fma(q[2], v, -(q[4] * o));
    if (!PRED || keep) s[0] = n1, s[1] = n2;
    return o;
}

/* acc + A x for a 2-vector, one FMA chain per row */
__device__ __forceinline__ void eq_mv_add(const double *__restrict__ A, const double *x, double *acc) {
    const double r0 = fma(A[1], x[1], fma(A[0], x[0], acc[0]));
    const double r1 = fma(A[3], x[1], fma(A[2], x[0], acc[1]));
    acc[0] = r0, acc[1] = r1;
}

__global__ void __launch_bounds__(MP3D_EQ_THREADS)
k_eq_plan(EqState *__restrict__ st, const int32_t *__restrict__ counts, EqPlan *__restrict__ plan,
          int32_t *__restrict__ out_count, int n, long long sample_stride, long long out_stride, int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_EQ_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    EqPlan P;
    P.pad_ = 0;
    if (c > out_stride) {
        P.n_in = 0, P.tiles = 0, P.restart = 1;
        out_count[s] = -1;
    } else {
        P.n_in = (int)c;
        P.tiles = (int)((c + MP3D_EQ_TILE - 1) / MP3D_EQ_TILE);
        P.restart = flush;
        out_count[s] = (int)c;
    }
    plan[s] = P;
    /* no sample, so no thread of k_eq_apply holds the last one */
    if (P.restart && P.tiles == 0) {
        for (int k = 0; k < 2 * MP3D_EQ_NS; k++) st[s].f[k / MP3D_EQ_NS][k % MP3D_EQ_NS] = 0.0;
    }
}

/* element e of a tile's interleaved samples in its thread's padded run */
template <int C> __device__ __forceinline__ float *eq_at(float (*sx)[MP3D_EQ_THREADS * MP3D_EQ_PAD], int e) {
    const int j = e / C, c = e - j * C;
    return &sx[c][(j / MP3D_EQ_SEG) * MP3D_EQ_PAD + j % MP3D_EQ_SEG];
}

/* the tile's m samples (row: its first element) into LDS, 16 bytes per load where the row allows */
template <int C>
__device__ __forceinline__ void eq_stage(const float *__restrict__ row, int m,
                                         float (*sx)[MP3D_EQ_THREADS * MP3D_EQ_PAD], int t) {
    const int ne = m * C;
    if (((uintptr_t)row & 15) == 0) {
        const int n4 = ne & ~3;
        for (int e = t * 4; e < n4; e += MP3D_EQ_THREADS * 4) {
            const float4 v = *(const float4 *)(row + e);
            *eq_at<C>(sx, e) = v.x;
            *eq_at<C>(sx, e + 1) = v.y;
            *eq_at<C>(sx, e + 2) = v.z;
            *eq_at<C>(sx, e + 3) = v.w;
        }
        if (n4 + t < ne) *eq_at<C>(sx, n4 + t) = row[n4 + t];
    } else {
        for (int e = t; e < ne; e += MP3D_EQ_THREADS) *eq_at<C>(sx, e) = row[e];
    }
}

/* ... and the tile's m results from LDS to the caller's row */
template <int C>
__device__ __forceinline__ void eq_unstage(float *__restrict__ row, int m,
                                           float (*sx)[MP3D_EQ_THREADS * MP3D_EQ_PAD], int t) {
    const int ne = m * C;
    if (((uintptr_t)row & 15) == 0) {
        const int n4 = ne & ~3;
        for (int e = t * 4; e < n4; e += MP3D_EQ_THREADS * 4) {
            float4 v;
            v.x = *eq_at<C>(sx, e);
            v.y = *eq_at<C>(sx, e + 1);
            v.z = *eq_at<C>(sx, e + 2);
            v.w = *eq_at<C>(sx, e + 3);
            *(float4 *)(row + e) = v;
        }
        if (n4 + t < ne) row[n4 + t] = *eq_at<C>(sx, n4 + t);
    } else {
        for (int e = t; e < ne; e += MP3D_EQ_THREADS) row[e] = *eq_at<C>(sx, e);
    }
}

/* One stage of the cascade over the tile: v, the thread's cnt samples per
 * channel (the stage's inputs), become its outputs.  E: the stage's state at
 * the tile's first sample.  Returns in f the stage's state after the thread's
 * last sample.  wt: this stage's buffer of wave totals. */
template <int C, bool PRED>
__device__ __forceinline__ void eq_stage_pass(double (*v)[MP3D_EQ_SEG], int cnt, const double *q,
                                              const double (*__restrict__ ap)[4], double (*wt)[C * 2], double (*E)[2],
                                              double (*f)[2], int t) {
    const int lane = t & 63, w = t >> 6;
    double z[C][2];
#pragma unroll
    for (int c = 0; c < C; c++) {
        z[c][0] = z[c][1] = 0.0;
#pragma unroll
        for (int i = 0; i < MP3D_EQ_SEG; i++) (void)eq_step<PRED>(v[c][i], z[c], q, i < cnt);
    }
    /* inclusive affine scan over the lanes of the wave, in registers: step d
     * adds A^(SEG d) times the value d lanes back */
    for (int d = 1; d < 64; d <<= 1) {
        double y[C][2];
#pragma unroll
        for (int c = 0; c < C; c++) {
            y[c][0] = __shfl_up(z[c][0], (unsigned)d);
            y[c][1] = __shfl_up(z[c][1], (unsigned)d);
        }
        if (lane >= d) {
#pragma unroll
            for (int c = 0; c < C; c++) eq_mv_add(ap[d], y[c], z[c]);
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c < C; c++) wt[w][c * 2] = z[c][0], wt[w][c * 2 + 1] = z[c][1];
    }
    __syncthreads();
    /* the state at the wave's first sample: E <- A^(64 SEG) E + T_u over the waves before */
    for (int u = 0; u < w; u++) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            double y[2] = {wt[u][c * 2], wt[u][c * 2 + 1]};
            eq_mv_add(ap[64], E[c], y);
            E[c][0] = y[0], E[c][1] = y[1];
        }
    }
    /* ... and at the thread's: through A^(SEG lane), plus the scan value of the lane before */
#pragma unroll
    for (int c = 0; c < C; c++) {
        const double u0 = __shfl_up(z[c][0], 1u), u1 = __shfl_up(z[c][1], 1u);
        f[c][0] = lane ? u0 : 0.0;
        f[c][1] = lane ? u1 : 0.0;
        eq_mv_add(ap[lane], E[c], f[c]);
#pragma unroll
        for (int i = 0; i < MP3D_EQ_SEG; i++) v[c][i] = eq_step<PRED>(v[c][i], f[c], q, i < cnt);
    }
}

/* The cascade over a tile of m samples staged in sx.  entry: the tile's entry
 * state ([channel][MP3D_EQ_NS]) or null for zero.  endst: where the thread
 * with `last` stores every stage's state after its last sample (zeros when
 * `zero`), or null.  Afterwards sx holds the results as float32 when `emit`. */
template <int C>
__device__ __forceinline__ void eq_cascade(float (*sx)[MP3D_EQ_THREADS * MP3D_EQ_PAD],
                                           double (*wt)[MP3D_EQ_WAVES][C * 2], const EqTab *__restrict__ tab,
                                           const double *__restrict__ entry, double *__restrict__ endst, bool last,
                                           bool zero, bool emit, int m, int t) {
    const int cnt = max(0, min(MP3D_EQ_SEG, m - t * MP3D_EQ_SEG));
    const int K = tab->K;
    double v[C][MP3D_EQ_SEG];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float *p = sx[c] + t * MP3D_EQ_PAD;
#pragma unroll
        for (int i = 0; i < MP3D_EQ_SEG; i++) v[c][i] = i < cnt ? (double)p[i] : 0.0;
    }
    for (int k = 0; k < K; k++) {
        double q[5];
#pragma unroll
        for (int i = 0; i < 5; i++) q[i] = tab->coef[5 * k + i];
        double E[C][2], f[C][2];
#pragma unroll
        for (int c = 0; c < C; c++) {
            E[c][0] = entry ? entry[c * MP3D_EQ_NS + 2 * k] : 0.0;
            E[c][1] = entry ? entry[c * MP3D_EQ_NS + 2 * k + 1] : 0.0;
        }
        if (m == MP3D_EQ_TILE) /* (the whole block: no thread has a short segment) */
            eq_stage_pass<C, false>(v, cnt, q, tab->apow[k], wt[k & 1], E, f, t);
        else
            eq_stage_pass<C, true>(v, cnt, q, tab->apow[k], wt[k & 1], E, f, t);
        if (endst && last) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                endst[c * MP3D_EQ_NS + 2 * k] = zero ? 0.0 : f[c][0];
                endst[c * MP3D_EQ_NS + 2 * k + 1] = zero ? 0.0 : f[c][1];
            }
        }
    }
    if (emit) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            float *p = sx[c] + t * MP3D_EQ_PAD;
#pragma unroll
            for (int i = 0; i < MP3D_EQ_SEG; i++)
                if (i < cnt) p[i] = (float)v[c][i];
        }
    }
}

/* z_TILE of every tile that another tile follows */
template <int C>
__global__ void __launch_bounds__(MP3D_EQ_THREADS)
k_eq_local(const float *__restrict__ samples, const EqPlan *__restrict__ plan, const EqTab *__restrict__ tab,
           double *__restrict__ tz, long long sample_stride, int tiles) {
    __shared__ __attribute__((aligned(16))) float sx[C][MP3D_EQ_THREADS * MP3D_EQ_PAD];
    __shared__ double wt[2][MP3D_EQ_WAVES][C * 2];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const EqPlan P = plan[s];
    if (tile + 1 >= P.tiles) return; /* (the last tile's end state comes from k_eq_apply) */
    const float *row = samples + ((size_t)s * (size_t)sample_stride + (size_t)tile * MP3D_EQ_TILE) * C;
    eq_stage<C>(row, MP3D_EQ_TILE, sx, t);
    __syncthreads();
    eq_cascade<C>(sx, wt, tab, nullptr, tz + ((size_t)s * tiles + tile) * MP3D_EQ_TSTRIDE, t == MP3D_EQ_THREADS - 1,
                  false, false, MP3D_EQ_TILE, t);
}

/* Every tile's entry state of one stream and channel: the slot's state, then
 * s <- A^TILE s + z_t.  64 tiles at a time: lane i holds z of tile base + i,
 * an affine scan over the lanes with A^(TILE 2^k) gives the state after each
 * tile for a zero entry, and A^(TILE i) carries the chunk's entry state to
 * lane i.  The vectors have 2K entries, K the caller's, so they live in LDS
 * rows (a row per lane, two buffers in turn) and not in registers.  A wave per
 * stage: wave g computes the stage's two rows 2g, 2g + 1 of every product, and
 * of their columns only the first 2g + 2 (the matrices are block lower
 * triangular, the rest is exact zeros).  One stream's thousands of tiles cost
 * one such scan per 64, and a row's chain is at most 20 long. */
__global__ void __launch_bounds__(64 * MP3D_EQ_BANDS)
k_eq_carry(const EqState *__restrict__ st, const EqPlan *__restrict__ plan, const EqTab *__restrict__ tab,
           const double *__restrict__ tpow, const double *__restrict__ tz, double *__restrict__ entry, int tiles) {
    __shared__ double zb[2][64][MP3D_EQ_NS + 1];
    __shared__ double Es[2][MP3D_EQ_NS];
    MP3D_LDS_ENTRY();
    const int ch = tab->ch, s = blockIdx.x / ch, c = blockIdx.x % ch, t = threadIdx.x;
    const int lane = t & 63, r0 = 2 * (t >> 6), nc = r0 + 2; /* (the block has K waves) */
    const EqPlan P = plan[s];
    if (P.tiles <= 0) return;
    const int n = 2 * tab->K, nn = n * n;
    if (t < n) Es[0][t] = st[s].f[c][t];
    int eb = 0;
    for (int base = 0; base < P.tiles; base += 64) {
        const bool has = base + lane + 1 < P.tiles; /* (the last tile has no z: nothing follows it) */
        const double *zp = tz + ((size_t)s * tiles + base + (has ? lane : 0)) * MP3D_EQ_TSTRIDE + c * MP3D_EQ_NS;
        zb[0][lane][r0] = has ? zp[r0] : 0.0;
        zb[0][lane][r0 + 1] = has ? zp[r0 + 1] : 0.0;
        int cur = 0;
        __syncthreads();
        /* (a lane under m reads lanes under m only: no step past the chunk's tiles) */
        const int m = min(64, P.tiles - base);
        for (int d = 1; d < m; d <<= 1) {
            const double *A = tpow + (size_t)d * nn;
            for (int r = r0; r < r0 + 2; r++) {
                double acc = zb[cur][lane][r];
                if (lane >= d) {
#pragma unroll 4
                    for (int j = 0; j < nc; j++) acc = fma(A[r * n + j], zb[cur][lane - d][j], acc);
                }
                zb[cur ^ 1][lane][r] = acc;
            }
            cur ^= 1;
            __syncthreads();
        }
        /* the state before tile base + lane */
        if (base + lane < P.tiles) {
            const double *A = tpow + (size_t)lane * nn;
            double *o = entry + ((size_t)s * tiles + base + lane) * MP3D_EQ_TSTRIDE + c * MP3D_EQ_NS;
            for (int r = r0; r < r0 + 2; r++) {
                double acc = lane ? zb[cur][lane - 1][r] : 0.0;
#pragma unroll 4
                for (int j = 0; j < nc; j++) acc = fma(A[r * n + j], Es[eb][j], acc);
                o[r] = acc;
            }
        }
        if (base + 64 < P.tiles) { /* the next chunk's entry: after this chunk's last tile */
            const double *T = tpow + (size_t)64 * nn;
            if (lane < 2) {
                const int r = r0 + lane;
                double acc = zb[cur][63][r];
                for (int j = 0; j < nc; j++) acc = fma(T[r * n + j], Es[eb][j], acc);
                Es[eb ^ 1][r] = acc;
            }
            eb ^= 1;
        }
        __syncthreads();
    }
}

/* the call's samples through the cascade, from every tile's true entry state */
template <int C>
__global__ void __launch_bounds__(MP3D_EQ_THREADS)
k_eq_apply(const float *__restrict__ samples, const EqPlan *__restrict__ plan, const EqTab *__restrict__ tab,
           const double *__restrict__ entry, EqState *__restrict__ st, float *__restrict__ out,
           long long sample_stride, long long out_stride, int tiles) {
    __shared__ __attribute__((aligned(16))) float sx[C][MP3D_EQ_THREADS * MP3D_EQ_PAD];
    __shared__ double wt[2][MP3D_EQ_WAVES][C * 2];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const EqPlan P = plan[s];
    if (tile >= P.tiles) return;
    const int m = min(MP3D_EQ_TILE, P.n_in - tile * MP3D_EQ_TILE);
    const float *row = samples + ((size_t)s * (size_t)sample_stride + (size_t)tile * MP3D_EQ_TILE) * C;
    eq_stage<C>(row, m, sx, t);
    __syncthreads();
    const int cnt = max(0, min(MP3D_EQ_SEG, m - t * MP3D_EQ_SEG));
    const bool last = cnt > 0 && (long long)tile * MP3D_EQ_TILE + t * MP3D_EQ_SEG + cnt == P.n_in;
    eq_cascade<C>(sx, wt, tab, entry + ((size_t)s * tiles + tile) * MP3D_EQ_TSTRIDE, &st[s].f[0][0], last,
                  P.restart != 0, true, m, t);
    __syncthreads();
    eq_unstage<C>(out + ((size_t)s * (size_t)out_stride + (size_t)tile * MP3D_EQ_TILE) * C, m, sx, t);
}

void launch_eq(const float *samples, const int32_t *counts, EqState *st, EqPlan *plan, const EqTab *tab,
               const double *tpow, double *tz, double *entry, float *out, int32_t *out_count, int K, int ch, int n,
               long long sample_stride, long long out_stride, int tiles, int flush, hipStream_t strm) {
    const dim3 blk(MP3D_EQ_THREADS), grid((unsigned)n * (unsigned)tiles);
    hipLaunchKernelGGL(k_eq_plan, dim3((n + MP3D_EQ_THREADS - 1) / MP3D_EQ_THREADS), blk, 0, strm, st, counts, plan,
                       out_count, n, sample_stride, out_stride, flush);
    if (tiles > 1) { /* (a call whose streams fit one tile each has no z to compute) */
        if (ch == 2)
            hipLaunchKernelGGL(k_eq_local<2>, grid, blk, 0, strm, samples, plan, tab, tz, sample_stride, tiles);
        else
            hipLaunchKernelGGL(k_eq_local<1>, grid, blk, 0, strm, samples, plan, tab, tz, sample_stride, tiles);
    }
    hipLaunchKernelGGL(k_eq_carry, dim3((unsigned)n * (unsigned)ch), dim3(64 * K), 0, strm, st, plan, tab, tpow, tz,
                       entry, tiles);
    if (ch == 2)
        hipLaunchKernelGGL(k_eq_apply<2>, grid, blk, 0, strm, samples, plan, tab, entry, st, out, sample_stride,
                           out_stride, tiles);
    else
        hipLaunchKernelGGL(k_eq_apply<1>, grid, blk, 0, strm, samples, plan, tab, entry, st, out, sample_stride,
                           out_stride, tiles);
}

} // namespace mp3d
