/*
 * mp3d_loudness.hip -- the loudness sink: ITU-R BS.1770-4 K-weighting, 100 ms
 * block energies, sample peak and the gated integrated loudness of block rows
 * (include/mp3d.h "loudness sink"; mp3d_loudness.h has
 * the kernel list and the layouts).
 *
 * The K-weighting cascade is an IIR filter, so a stream's samples cannot be
 * dealt to threads as a feed-forward filter's can.  Its state is a 4-vector
 * per channel and one sample maps it affinely, s' = A s + B v, so a run of g
 * samples maps it as s_end = A^g s_start + z_g, with z_g the end state from a
 * zero start.  Every thread filters MP3D_LD_SEG samples from a zero state
 * (z of its segment), a log-step scan over the lanes of each wave with the
 * precomputed A^(SEG 2^k), in registers, turns those into the state at every
 * segment boundary for a zero wave entry, the waves' totals are walked through
 * A^(64 SEG) from the tile's true entry state (itself walked over the tiles by
 * k_ld_carry), and A^(SEG lane) carries that to the lane.  Each thread then
 * filters its segment again from its true entry state and squares the output.
 *
 * Everything after the float32 sample is double.  No floating-point atomics:
 * every sum has one fixed order (thread, group of 16 threads, tile), so the
 * same call on the same state gives the same bits.  Tiles are counted from
 * the call's first sample, block boundaries from the stream's restart, so a
 * stream fed in other pieces adds in another order: equal within the bound
 * of include/mp3d.h, not bit for bit.
 */
#include "mp3d_device.h"
#include "mp3d_loudness.h"
#include "mp3d_launch.h"

/* the wglds build and the product build must round alike: no implicit
 * contraction, every fused multiply-add below is written as fma */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_LD_TILE == MP3D_LD_THREADS * MP3D_LD_SEG && MP3D_LD_TILE <= 16384, "tile size of the contract");
static_assert(MP3D_LD_SEG < MP3D_LD_MIN_H, "a thread's segment touches at most two blocks");
static_assert(MP3D_LD_THREADS == 256, "four waves: their totals are walked in turn, their peaks joined by name");
#define MP3D_LD_GROUPS (MP3D_LD_THREADS / 16)
#define MP3D_LD_WAVES (MP3D_LD_THREADS / 64)
static_assert(MP3D_LD_GROUPS * MP3D_LD_TILE_BLOCKS <= MP3D_LD_THREADS, "one thread per (group, block) partial");
static_assert(2 * sizeof(double) <= MP3D_LD_PAD * sizeof(float), "the per-thread sums fit where a channel's samples were");

/* one sample through the cascade: s = {stage 1 s1, s2, stage 2 s1, s2},
 * c = {b0 b1 b2 a1 a2} of stage 1, then of stage 2; returns stage 2's output */
__device__ __forceinline__ double ld_step(double v, double *s, const double *c) {
    const double o1 = fma(c[0], v, s[0]);
    s[0] = fma(c[1], v, fma(-c[3], o1, s[1]));
    s[1] = fma(c[2], v, -(c[4] * o1));
    const double o2 = fma(c[5], o1, s[2]);
    s[2] = fma(c[6], o1, fma(-c[8], o2, s[3]));
    s[3] = fma(c[7], o1, -(c[9] * o2));
    return o2;
}

/* acc + A x for one channel's 4-vector, one FMA chain per row */
__device__ __forceinline__ void ld_mv_add(const double *__restrict__ A, const double *x, double *acc) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double a = acc[r];
#pragma unroll
        for (int j = 0; j < 4; j++) a = fma(A[r * 4 + j], x[j], a);
        acc[r] = a;
    }
}

__global__ void __launch_bounds__(MP3D_LD_THREADS)
k_ld_plan(const LdState *__restrict__ st, const int32_t *__restrict__ counts, LdPlan *__restrict__ plan,
          int32_t *__restrict__ block_count, int n, long long sample_stride, long long block_stride, int H, int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_LD_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    LdPlan P;
    P.n0 = st[s].n;
    P.n_in = (int)c;
    P.restart = flush;
    P.tiles = (int)((c + MP3D_LD_TILE - 1) / MP3D_LD_TILE);
    const long long k = (P.n0 + c) / H - P.n0 / H;
    if (k > block_stride) {
        P.count = -1;
        P.restart = 1;
    } else {
        P.count = (int)k;
    }
    plan[s] = P;
    block_count[s] = P.count;
}

/* element e of a tile's interleaved samples to its thread's padded run */
template <int C> __device__ __forceinline__ void ld_put(float (*sx)[MP3D_LD_THREADS * MP3D_LD_PAD], int e, float v) {
    const int j = e / C, c = e - j * C;
    sx[c][(j / MP3D_LD_SEG) * MP3D_LD_PAD + j % MP3D_LD_SEG] = v;
}

/* The tile's m samples (row: its first element) into LDS, 16 bytes per load
 * where the row allows; returns the largest |v| this thread loaded. */
template <int C>
__device__ __forceinline__ float ld_stage(const float *__restrict__ row, int m,
                                          float (*sx)[MP3D_LD_THREADS * MP3D_LD_PAD], int t) {
    const int ne = m * C;
    float pk = 0.0f;
    if (((uintptr_t)row & 15) == 0) {
        const int n4 = ne & ~3;
        for (int e = t * 4; e < n4; e += MP3D_LD_THREADS * 4) {
            const float4 v = *(const float4 *)(row + e);
            ld_put<C>(sx, e, v.x);
            ld_put<C>(sx, e + 1, v.y);
            ld_put<C>(sx, e + 2, v.z);
            ld_put<C>(sx, e + 3, v.w);
            pk = fmaxf(pk, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
        if (n4 + t < ne) {
            const float v = row[n4 + t];
            ld_put<C>(sx, n4 + t, v);
            pk = fmaxf(pk, fabsf(v));
        }
    } else {
        for (int e = t; e < ne; e += MP3D_LD_THREADS) {
            const float v = row[e];
            ld_put<C>(sx, e, v);
            pk = fmaxf(pk, fabsf(v));
        }
    }
    return pk;
}

/* thread t's cnt samples of every channel from a zero state: x = z of its segment */
template <int C>
__device__ __forceinline__ void ld_local_pass(float (*sx)[MP3D_LD_THREADS * MP3D_LD_PAD], int t, int cnt,
                                              const double *coef, double *x) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        const float *p = sx[c] + t * MP3D_LD_PAD;
        if (cnt == MP3D_LD_SEG) { /* (all of a full tile's threads) */
#pragma unroll
            for (int i = 0; i < MP3D_LD_SEG; i++) (void)ld_step((double)p[i], s, coef);
        } else {
            for (int i = 0; i < cnt; i++) (void)ld_step((double)p[i], s, coef);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) x[c * 4 + r] = s[r];
    }
}

/* Inclusive affine scan over the lanes of a wave, in registers: afterwards x
 * is the state at the end of the lane's segment when the wave's first segment
 * is entered with a zero state.  Step d adds A^(SEG d) times the value d lanes
 * back.  No barrier: the block's scan cost 16 of them and left two waves per
 * SIMD waiting on each other. */
template <int C> __device__ __forceinline__ void ld_wave_scan(double *x, const LdTab *__restrict__ tab, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        double y[C * 4];
#pragma unroll
        for (int k = 0; k < C * 4; k++) y[k] = __shfl_up(x[k], (unsigned)d);
        if (lane >= d) {
            const double *A = tab->apow[d];
#pragma unroll
            for (int c = 0; c < C; c++) ld_mv_add(A, y + c * 4, x + c * 4);
        }
    }
}

/* E <- A^(64 SEG) E + T_u for the waves u = 0 .. w - 1 in turn: from the
 * state at the tile's first sample to the state at wave w's first sample;
 * wt[u] is wave u's total (its last lane's scan value) */
template <int C>
__device__ __forceinline__ void ld_wave_walk(double (*wt)[8], double *E, const LdTab *__restrict__ tab, int w) {
    const double *A = tab->apow[64];
    for (int u = 0; u < w; u++) {
        double y[C * 4];
#pragma unroll
        for (int k = 0; k < C * 4; k++) y[k] = wt[u][k];
#pragma unroll
        for (int c = 0; c < C; c++) ld_mv_add(A, E + c * 4, y + c * 4);
#pragma unroll
        for (int k = 0; k < C * 4; k++) E[k] = y[k];
    }
}

/* z_TILE of every tile that another tile follows */
template <int C>
__global__ void __launch_bounds__(MP3D_LD_THREADS)
k_ld_local(const float *__restrict__ samples, const LdPlan *__restrict__ plan, const LdTab *__restrict__ tab,
           double *__restrict__ tz, long long sample_stride, int tiles) {
    __shared__ __attribute__((aligned(16))) float sx[C][MP3D_LD_THREADS * MP3D_LD_PAD];
    __shared__ double wt[MP3D_LD_WAVES][8];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const LdPlan P = plan[s];
    if (tile + 1 >= P.tiles) return; /* (the last tile's end state comes from k_ld_energy) */
    const float *row = samples + ((size_t)s * (size_t)sample_stride + (size_t)tile * MP3D_LD_TILE) * C;
    (void)ld_stage<C>(row, MP3D_LD_TILE, sx, t);
    __syncthreads();
    double coef[10];
#pragma unroll
    for (int i = 0; i < 10; i++) coef[i] = tab->coef[i];
    double x[C * 4];
    ld_local_pass<C>(sx, t, MP3D_LD_SEG, coef, x);
    ld_wave_scan<C>(x, tab, t & 63);
    if ((t & 63) == 63) {
#pragma unroll
        for (int k = 0; k < C * 4; k++) wt[t >> 6][k] = x[k];
    }
    __syncthreads();
    if (t == 0) {
        double E[C * 4];
#pragma unroll
        for (int k = 0; k < C * 4; k++) E[k] = 0.0;
        ld_wave_walk<C>(wt, E, tab, MP3D_LD_WAVES);
        double *o = tz + ((size_t)s * tiles + tile) * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = k < C * 4 ? E[k < C * 4 ? k : 0] : 0.0;
    }
}

/* Every tile's entry state: the slot's state, then s <- A^TILE s + z_t.  64
 * tiles at a time: lane i holds z of tile base + i, an affine scan over the
 * lanes with A^(TILE 2^k) gives the state after each tile for a zero entry,
 * and A^(TILE i) carries the chunk's entry state E to lane i.  One long
 * stream's thousands of tiles cost one such scan per 64, not a dependent
 * step each. */
__global__ void __launch_bounds__(64)
k_ld_carry(const LdState *__restrict__ st, const LdPlan *__restrict__ plan, const LdTab *__restrict__ tab,
           const double *__restrict__ tz, double *__restrict__ entry, int tiles) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, lane = threadIdx.x;
    const LdPlan P = plan[s];
    if (P.tiles <= 0) return;
    double E[8];
#pragma unroll
    for (int k = 0; k < 8; k++) E[k] = st[s].f[k / 4][k % 4];
    for (int base = 0; base < P.tiles; base += 64) {
        double z[8];
        const bool has = base + lane + 1 < P.tiles; /* (the last tile has no z: nothing follows it) */
        const double *zp = tz + ((size_t)s * tiles + base + (has ? lane : 0)) * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) z[k] = has ? zp[k] : 0.0;
        for (int d = 1; d < 64; d <<= 1) {
            double y[8];
#pragma unroll
            for (int k = 0; k < 8; k++) y[k] = __shfl_up(z[k], (unsigned)d);
            if (lane >= d) {
                const double *A = tab->tpow[d];
                ld_mv_add(A, y, z);
                ld_mv_add(A, y + 4, z + 4);
            }
        }
        /* the state before tile base + lane */
        double f[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double up = __shfl_up(z[k], 1u);
            f[k] = lane ? up : 0.0;
        }
        const double *A = tab->tpow[lane];
        ld_mv_add(A, E, f);
        ld_mv_add(A, E + 4, f + 4);
        if (base + lane < P.tiles) {
            double *o = entry + ((size_t)s * tiles + base + lane) * 8;
#pragma unroll
            for (int k = 0; k < 8; k++) o[k] = f[k];
        }
        if (base + 64 < P.tiles) { /* the next chunk's entry: after this chunk's last tile */
            double y[8];
#pragma unroll
            for (int k = 0; k < 8; k++) y[k] = __shfl(z[k], 63);
            const double *T = tab->tpow[64];
            ld_mv_add(T, E, y);
            ld_mv_add(T, E + 4, y + 4);
#pragma unroll
            for (int k = 0; k < 8; k++) E[k] = y[k];
        }
    }
}

/* per-(tile, block) sums of y^2 over the channels, the tile's peak, and from
 * the thread that holds the call's last sample the filter state after it */
template <int C>
__global__ void __launch_bounds__(MP3D_LD_THREADS)
k_ld_energy(const float *__restrict__ samples, const LdPlan *__restrict__ plan, const LdTab *__restrict__ tab,
            const double *__restrict__ entry, double *__restrict__ part, float *__restrict__ tpeak,
            double *__restrict__ endst, long long sample_stride, int tiles) {
    __shared__ __attribute__((aligned(16))) float sx[C][MP3D_LD_THREADS * MP3D_LD_PAD];
    __shared__ double wt[MP3D_LD_WAVES][8];
    __shared__ double r2[MP3D_LD_GROUPS][MP3D_LD_TILE_BLOCKS];
    __shared__ int rk[MP3D_LD_THREADS];
    __shared__ float pks[MP3D_LD_WAVES];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const LdPlan P = plan[s];
    if (tile >= P.tiles) return;
    const int m = min(MP3D_LD_TILE, P.n_in - tile * MP3D_LD_TILE);
    const float *row = samples + ((size_t)s * (size_t)sample_stride + (size_t)tile * MP3D_LD_TILE) * C;
    float pk = ld_stage<C>(row, m, sx, t);
    __syncthreads();
    double coef[10];
#pragma unroll
    for (int i = 0; i < 10; i++) coef[i] = tab->coef[i];
    const int cnt = max(0, min(MP3D_LD_SEG, m - t * MP3D_LD_SEG));
    double x[C * 4];
    ld_local_pass<C>(sx, t, cnt, coef, x);
    const int lane = t & 63;
    ld_wave_scan<C>(x, tab, lane);
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < C * 4; k++) wt[t >> 6][k] = x[k];
    }
    __syncthreads();

    /* the true state at this thread's first sample: the tile's entry state
     * walked to the wave's first sample, then through the lane's A^(SEG lane),
     * plus the scan value of the lane before */
    double E[C * 4];
    const double *e = entry + ((size_t)s * tiles + tile) * 8;
#pragma unroll
    for (int k = 0; k < C * 4; k++) E[k] = e[k];
    ld_wave_walk<C>(wt, E, tab, t >> 6);
    const double *A = tab->apow[lane];
    double f[C][4];
#pragma unroll
    for (int c = 0; c < C; c++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double up = __shfl_up(x[c * 4 + r], 1u);
            f[c][r] = lane ? up : 0.0;
        }
        ld_mv_add(A, E + c * 4, f[c]);
    }

    /* blocks are counted from the stream's restart */
    const int H = tab->H;
    const long long g0 = P.n0 + (long long)tile * MP3D_LD_TILE + t * MP3D_LD_SEG;
    const long long blk = g0 / H, first = (P.n0 + (long long)tile * MP3D_LD_TILE) / H;
    const int ib = (int)((blk + 1) * H - g0); /* samples from here on lie in the next block */
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float *p = sx[c] + t * MP3D_LD_PAD;
        if (cnt == MP3D_LD_SEG) { /* (all of a full tile's threads) */
#pragma unroll
            for (int i = 0; i < MP3D_LD_SEG; i++) {
                const double y = ld_step((double)p[i], f[c], coef);
                if (i < ib) sa = fma(y, y, sa);
                else sb = fma(y, y, sb);
            }
        } else {
            for (int i = 0; i < cnt; i++) {
                const double y = ld_step((double)p[i], f[c], coef);
                if (i < ib) sa = fma(y, y, sa);
                else sb = fma(y, y, sb);
            }
        }
    }
    if (cnt > 0 && tile * MP3D_LD_TILE + t * MP3D_LD_SEG + cnt == P.n_in) {
        double *o = endst + (size_t)s * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = k < C * 4 ? f[k / 4 < C ? k / 4 : 0][k % 4] : 0.0;
    }

    /* fixed order: 16 threads in turn, then the 16 groups in turn.  The
     * per-thread sums take the place of the samples, which nobody reads again. */
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d)); /* (a maximum: any order) */
    if (lane == 0) pks[t >> 6] = pk;
    __syncthreads();
    double *ra = (double *)&sx[0][0], *rb = ra + MP3D_LD_THREADS;
    ra[t] = sa;
    rb[t] = sb;
    rk[t] = (int)(blk - first);
    __syncthreads();
    if (t < MP3D_LD_GROUPS * MP3D_LD_TILE_BLOCKS) {
        const int q = t / MP3D_LD_TILE_BLOCKS, k = t - q * MP3D_LD_TILE_BLOCKS;
        double acc = 0.0;
        for (int u = q * 16; u < q * 16 + 16; u++) {
            const int kk = rk[u];
            acc += kk == k ? ra[u] : 0.0;
            acc += kk + 1 == k ? rb[u] : 0.0;
        }
        r2[q][k] = acc;
    }
    __syncthreads();
    if (t < MP3D_LD_TILE_BLOCKS) {
        double acc = 0.0;
        for (int q = 0; q < MP3D_LD_GROUPS; q++) acc += r2[q][t];
        part[((size_t)s * tiles + tile) * MP3D_LD_TILE_BLOCKS + t] = acc;
    }
    if (t == 0) tpeak[(size_t)s * tiles + tile] = fmaxf(fmaxf(pks[0], pks[1]), fmaxf(pks[2], pks[3]));
}

/* the call's complete blocks, its count and peak, and the state after it */
__global__ void __launch_bounds__(64)
k_ld_finish(LdState *__restrict__ st, const LdPlan *__restrict__ plan, const LdTab *__restrict__ tab,
            const double *__restrict__ part, const float *__restrict__ tpeak, const double *__restrict__ endst,
            float *__restrict__ blocks, long long block_stride, float *__restrict__ peak, int tiles) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x;
    const LdPlan P = plan[s];
    const long long H = tab->H;
    const double carried = st[s].part;
    __syncthreads(); /* every read of the old state is before the new one's stores */

    float pk = 0.0f;
    for (int i = t; i < P.tiles; i += 64) pk = fmaxf(pk, tpeak[(size_t)s * tiles + i]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d));
    if (t == 0 && peak) peak[s] = pk;

    const long long n0 = P.n0, n1 = n0 + P.n_in, b0 = n0 / H, nb = n1 / H - b0;
    /* j = nb is the open block: its sum goes on in the state */
    for (long long j = t; j <= nb; j += 64) {
        const long long b = b0 + j;
        const long long lo = (b * H > n0 ? b * H : n0) - n0, hi = ((b + 1) * H < n1 ? (b + 1) * H : n1) - n0;
        double sum = j == 0 ? carried : 0.0;
        if (hi > lo)
            for (long long i = lo / MP3D_LD_TILE; i <= (hi - 1) / MP3D_LD_TILE; i++) {
                const long long first = (n0 + i * MP3D_LD_TILE) / H;
                sum += part[((size_t)s * tiles + (size_t)i) * MP3D_LD_TILE_BLOCKS + (size_t)(b - first)];
            }
        if (j < nb) {
            if (P.count >= 0) blocks[(size_t)s * (size_t)block_stride + (size_t)j] = (float)(sum / (double)H);
            continue;
        }
        LdState *S = st + s;
        if (P.restart) {
            S->n = 0;
            S->part = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) S->f[k / 4][k % 4] = 0.0;
        } else if (P.n_in) {
            S->n = n1;
            S->part = n1 % H ? sum : 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) S->f[k / 4][k % 4] = endst[(size_t)s * 8 + k];
        }
    }
}

/* sum over the wave, the same bits in every lane (a + b = b + a) */
__device__ __forceinline__ double ld_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

/* gated integrated loudness of one row of blocks per wave */
__global__ void __launch_bounds__(64)
k_ld_gate(const float *__restrict__ blocks, long long block_stride, const int32_t *__restrict__ counts,
          float *__restrict__ lufs) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x;
    long long c = counts[s];
    c = c > block_stride ? block_stride : c;
    if (c < 4) {
        if (t == 0) lufs[s] = -INFINITY;
        return;
    }
    const float *z = blocks + (size_t)s * (size_t)block_stride;
    const long long m = c - 3;
    double s1 = 0.0, c1 = 0.0;
    for (long long j = t; j < m; j += 64) {
        const double G = ((double)z[j] + (double)z[j + 1] + (double)z[j + 2] + (double)z[j + 3]) / 4.0;
        if (-0.691 + 10.0 * log10(G) > -70.0) {
            s1 += G;
            c1 += 1.0;
        }
    }
    s1 = ld_wave_sum(s1);
    c1 = ld_wave_sum(c1);
    if (c1 == 0.0) {
        if (t == 0) lufs[s] = -INFINITY;
        return;
    }
    const double gamma = -0.691 + 10.0 * log10(s1 / c1) - 10.0;
    double s2 = 0.0, c2 = 0.0;
    for (long long j = t; j < m; j += 64) {
        const double G = ((double)z[j] + (double)z[j + 1] + (double)z[j + 2] + (double)z[j + 3]) / 4.0;
        const double l = -0.691 + 10.0 * log10(G);
        if (l > -70.0 && l > gamma) {
            s2 += G;
            c2 += 1.0;
        }
    }
    s2 = ld_wave_sum(s2);
    c2 = ld_wave_sum(c2);
    if (t == 0) lufs[s] = c2 == 0.0 ? -INFINITY : (float)(-0.691 + 10.0 * log10(s2 / c2));
}

void launch_loudness(const float *samples, const int32_t *counts, LdState *st, LdPlan *plan, const LdTab *tab, int H,
                     int ch, double *tz, double *entry, double *part, float *tpeak, double *endst, float *blocks,
                     int32_t *block_count, float *peak, int n, long long sample_stride, long long block_stride,
                     int tiles, int flush, hipStream_t strm) {
    const dim3 blk(MP3D_LD_THREADS), wave(64), grid((unsigned)n * (unsigned)tiles);
    hipLaunchKernelGGL(k_ld_plan, dim3((n + MP3D_LD_THREADS - 1) / MP3D_LD_THREADS), blk, 0, strm, st, counts, plan,
                       block_count, n, sample_stride, block_stride, H, flush);
    if (tiles > 1) {
        if (ch == 2)
            hipLaunchKernelGGL(k_ld_local<2>, grid, blk, 0, strm, samples, plan, tab, tz, sample_stride, tiles);
        else
            hipLaunchKernelGGL(k_ld_local<1>, grid, blk, 0, strm, samples, plan, tab, tz, sample_stride, tiles);
    }
    hipLaunchKernelGGL(k_ld_carry, dim3(n), wave, 0, strm, st, plan, tab, tz, entry, tiles);
    if (ch == 2)
        hipLaunchKernelGGL(k_ld_energy<2>, grid, blk, 0, strm, samples, plan, tab, entry, part, tpeak, endst,
                           sample_stride, tiles);
    else
        hipLaunchKernelGGL(k_ld_energy<1>, grid, blk, 0, strm, samples, plan, tab, entry, part, tpeak, endst,
                           sample_stride, tiles);
    hipLaunchKernelGGL(k_ld_finish, dim3(n), wave, 0, strm, st, plan, tab, part, tpeak, endst, blocks, block_stride,
                       peak, tiles);
}

void launch_loudness_gate(const float *blocks, long long block_stride, const int32_t *counts, float *lufs, int n,
                          hipStream_t strm) {
    hipLaunchKernelGGL(k_ld_gate, dim3(n), dim3(64), 0, strm, blocks, block_stride, counts, lufs);
}

} // namespace mp3d
