/*
 * mp3d_limiter.hip -- the look-ahead true-peak limiter: a per-sample gain on
 * packed float32 samples that holds the 4x oversampled peak of every sample
 * frame under a ceiling (include/mp3d.h "limiter"; DESIGN.md section 4h;
 * mp3d_limiter.h has the kernel list, the layouts and the LDS budget).
 *
 * Every value is one float32 rounding or exact integer arithmetic, so the
 * output has one value whatever call, tile or lane computes it:
 *   v      = fl(x * gain[s])
 *   p[i]   = max_c,p |u_c[4i + p]|, u the true-peak tap's FMA chain on v
 *   R[i]   = p <= c ? 2^20 : (int) floorf(fl(c / p) * 2^20)
 *   m[k]   = min R[k - 2A .. k + A]                       (int32)
 *   G[i]   = (sum_{j <= A} m[i - j]) / (A + 1)            (int32, truncated)
 *   y      = fl(v * (float)G * 2^-20)
 * The gain envelope is FIR, so a tile needs nothing from its neighbour but
 * samples: a halo of 3A + 5 frames back and A + 6 ahead, recomputed.
 *
 * Mapping (k_lim_tile): one 384-thread block per (stream, tile of 4096 emitted
 * indices).  The span goes into LDS in the tap's padded runs of 16 frames; a
 * thread runs the chains of 16 consecutive indices from a register window
 * (mp3d_tp_chain.h) and writes their R into ra[], which is padded the same
 * way (a word skipped after every 16) so that the stores of a run and the
 * reads of the minimum, 16 consecutive words per thread at a stride of 17,
 * spread over the banks.  The same thread then owns the run's 16 minima: the
 * sliding minimum and the running sum never leave its registers in between.
 */
#include "mp3d_device.h"
#include "mp3d_limiter.h"
#include "mp3d_tp_chain.h"
#include "mp3d_launch.h"

/* the wglds build and the product build must round alike: no contraction */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_LIM_THREADS % 64 == 0 && MP3D_LIM_THREADS % MP3D_TP_SEG == 0, "whole waves; a thread's strided words keep their place in a run");
static_assert(MP3D_TP_SEG == 16 && MP3D_TP_PAD == 17, "RA() pads a run of 16 to 17");
static_assert(MP3D_LIM_NR >= MP3D_LIM_TILE + 4 * MP3D_LIM_AMAX, "every required gain of a tile has a word");
static_assert(MP3D_LIM_THREADS * MP3D_TP_SEG >= MP3D_LIM_TILE + 4 * MP3D_LIM_AMAX, "one round of chains");
static_assert(MP3D_LIM_THREADS * MP3D_LIM_PSEG >= MP3D_LIM_TILE + MP3D_LIM_AMAX, "every minimum has a thread");
static_assert((long long)(MP3D_LIM_AMAX + 1) * MP3D_LIM_Q < 0x7fffffffLL, "the box sum fits int32");
static_assert(MP3D_LIM_NR == MP3D_LIM_THREADS * MP3D_TP_SEG && MP3D_LIM_PSEG == MP3D_TP_SEG, "thread t has run t, of R and of the minima");
static_assert(3 * MP3D_LIM_AMAX / 16 - 1 < 4 * 32, "L2 <= 64: its last step reads 32 words ahead");
static_assert((MP3D_LIM_TILE + MP3D_LIM_AMAX + 15) / 16 + 3 * MP3D_LIM_AMAX / 16 + 1 <= MP3D_LIM_NR / 16, "the runs a thread with minima reads");
#define MP3D_LIM_WAVES (MP3D_LIM_THREADS / 64)
#define MP3D_LIM_LOADS 8 /* global loads a thread has in flight while it stages */
/* word of required gain / minimum / running sum e in ra[] */
#define RA(e) ((e) + ((e) >> 4))
/* NR words in padded runs and one run more (the run after the one a window ends in is read whole) */
#define MP3D_LIM_RAW ((MP3D_LIM_NR / 16 + 1) * MP3D_TP_PAD)
/* INT_MAX words behind the run minima, as far as their last doubling step reads */
#define MP3D_LIM_DPAD 32

__global__ void __launch_bounds__(MP3D_LIM_THREADS)
k_lim_plan(const LimState *__restrict__ st, const int32_t *__restrict__ counts, LimPlan *__restrict__ plan,
           int32_t *__restrict__ out_count, int n, long long sample_stride, long long out_stride, int A, int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_LIM_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    LimPlan P;
    P.n0 = st[s].n;
    P.n_in = (int32_t)c;
    /* index i is emitted once sample i + A + 6 was seen; a flush emits the rest */
    const long long D = MP3D_LIM_AHEAD(A), n1 = P.n0 + c;
    const long long e1 = flush ? n1 : n1 > D ? n1 - D : 0;
    P.e0 = P.n0 > D ? P.n0 - D : 0;
    const long long n_emit = e1 - P.e0;
    const bool over = n_emit > out_stride;
    P.n_emit = over ? 0 : (int32_t)n_emit;
    P.tiles = (P.n_emit + MP3D_LIM_TILE - 1) / MP3D_LIM_TILE;
    P.restart = flush || over;
    plan[s] = P;
    out_count[s] = over ? -1 : (int32_t)n_emit;
}

/* The stream's pre-gained samples by their frame index RELATIVE TO THE CALL'S
 * FIRST (32 bits: a tile reaches K = 4A + 11 frames back at most): [-K, 0)
 * from the carry, [0, n_in) from the call, zeros before the stream's first
 * sample (first = max(-n0, -K)) and from n_in on. */
template <int C> struct LimSrc {
    const float *row, *carry, *gain;
    int first, n_in, K;
    float g;
    __device__ __forceinline__ LimSrc(const float *row_, const float *carry_, const float *gain_, int s,
                                      const LimPlan &P, int A)
        : row(row_), carry(carry_), gain(gain_), n_in(P.n_in), K(MP3D_LIM_BACK(A) + MP3D_LIM_AHEAD(A)),
          g(gain_ ? gain_[s] : 1.0f) {
        first = P.n0 < K ? -(int)P.n0 : -K;
    }
    /* element c of frame i, without a branch around the load (the address of
     * an element outside the stream is the carry's first), so that a round of
     * them is in flight together */
    __device__ __forceinline__ float at(int i, int c, bool want) const {
        const bool ok = want && i >= first && i < n_in, old = i < 0;
        /* (64 bits: n_in reaches 2^31 - 1 - 8192 frames, of C elements each) */
        const long long off = (long long)(old ? i + K : i) * C + c;
        const float *p = old ? carry : row;
        const float x = *(ok ? p + off : carry);
        const float v = old || !gain ? x : x * g;
        return ok ? v : 0.0f;
    }
    /* elements [0, E) of the frames from `base` on to put(e, v), MP3D_LIM_LOADS loads per thread at a time */
    template <class Put> __device__ __forceinline__ void each(int base, int E, int t, Put put) const {
        for (int e0 = t; e0 < E; e0 += MP3D_LIM_THREADS * MP3D_LIM_LOADS) {
            float v[MP3D_LIM_LOADS];
#pragma unroll
            for (int u = 0; u < MP3D_LIM_LOADS; u++) {
                /* a lane past E takes element E - 1's place and drops the value: base + j never
                 * passes the last frame asked for, at most n_in + A + 6 <= 2^31 - 1 - 8192 + 486 */
                const int ee = e0 + u * MP3D_LIM_THREADS, e = min(ee, E - 1), j = e / C;
                v[u] = at(base + j, e - j * C, ee < E);
            }
#pragma unroll
            for (int u = 0; u < MP3D_LIM_LOADS; u++)
                if (e0 + u * MP3D_LIM_THREADS < E) put(e0 + u * MP3D_LIM_THREADS, v[u]);
        }
    }
};

template <int C, bool F32> struct LimOut;
template <> struct LimOut<1, true> {
    typedef float T;
    static __device__ __forceinline__ T of(const float *v, float g) { return v[0] * g; }
};
template <> struct LimOut<2, true> {
    typedef float2 T;
    static __device__ __forceinline__ T of(const float *v, float g) { return make_float2(v[0] * g, v[1] * g); }
};
template <> struct LimOut<1, false> {
    typedef short T;
    static __device__ __forceinline__ T of(const float *v, float g) { return pcm_i16(v[0] * g); }
};
template <> struct LimOut<2, false> {
    typedef short2 T;
    static __device__ __forceinline__ T of(const float *v, float g) {
        return make_short2(pcm_i16(v[0] * g), pcm_i16(v[1] * g));
    }
};

template <int C, bool F32>
__global__ void __launch_bounds__(MP3D_LIM_THREADS)
k_lim_tile(const float *__restrict__ samples, const LimState *__restrict__ st, const LimPlan *__restrict__ plan,
           const float *__restrict__ taps, const float *__restrict__ gain, void *__restrict__ out,
           float *__restrict__ tilemin, long long sample_stride, long long out_stride, int tiles, int A, float c) {
    __shared__ __attribute__((aligned(16))) float sx[MP3D_LIM_RUNS * MP3D_TP_PAD * C];
    __shared__ int ra[MP3D_LIM_RAW];
    __shared__ int dbl[2][MP3D_LIM_THREADS + MP3D_LIM_DPAD];
    __shared__ unsigned wtot[MP3D_LIM_WAVES];
    __shared__ float wmin[MP3D_LIM_WAVES];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const LimPlan P = plan[s];
    if (tile >= P.tiles) return;
    const int m = min(MP3D_LIM_TILE, P.n_emit - tile * MP3D_LIM_TILE);
    /* the tile's first index, counted from the call's first sample (>= -(A + 6)) */
    const int o0 = (int)(P.e0 - P.n0) + tile * MP3D_LIM_TILE;
    const LimSrc<C> X(samples + (size_t)s * (size_t)sample_stride * C, st[s].carry, gain, s, P, A);

    /* the span: frames [o0 - 3A - 5, o0 + m + A + 6) */
    const int span = m + X.K;
    X.each(o0 - MP3D_LIM_BACK(A), span * C, t, [&](int e, float v) { tp_put<C>(sx, e, v); });
    const int nR = m + 4 * A;
    __syncthreads();

    /* R of indices [o0 - 3A, o0 + m + A): R[r] is the chain on span frames r .. r + 11;
     * thread t has run t of 16 and keeps the run's minimum (INT_MAX for a run past the last R) */
    int rm = 0x7fffffff;
    if (t * MP3D_TP_SEG < nR) {
        float tp[MP3D_TP_R - 1][MP3D_TP_TAPS];
        tp_load_taps(taps, tp);
        typedef typename TpFrame<C>::T T;
        const int cnt = min(MP3D_TP_SEG, nR - t * MP3D_TP_SEG);
        const int r0 = o0 - 3 * A + t * MP3D_TP_SEG;
        T w[MP3D_TP_SEG + MP3D_TP_HIST];
        tp_window<C>((const T *)sx + t * MP3D_TP_PAD, cnt + MP3D_TP_HIST, w);
#pragma unroll
        for (int i = 0; i < MP3D_TP_SEG; i++) {
            const float pk = tp_chain3<C>(w + i, tp);
            int R = MP3D_LIM_Q;
            /* (an IEEE division; a NaN peak compares false and leaves Q) */
            if (r0 + i >= X.first && r0 + i < X.n_in && pk > c) R = (int)floorf((c / pk) * 1048576.0f);
            if (i < cnt) {
                ra[t * MP3D_TP_PAD + i] = R;
                rm = min(rm, R);
            }
        }
    }
    /* The window of 3A + 1 values from q = 16 t + u on is the end of run t
     * from u on, the whole runs t + 1 .. t + k0 - 1, and R[16 (t + k0) ..
     * 16 (t + k0) + p0 + u], with k0 = 3A / 16 and p0 = 3A % 16: a running
     * minimum over u.  The whole runs' minimum is two overlapping spans of L2
     * run minima, L2 the largest power of two <= k0 - 1, from log2(L2)
     * doubling steps on the run minima, a word per thread, from one buffer
     * into the other. */
    const int k0 = (3 * A) >> 4, p0 = (3 * A) & 15;
    int L2 = 1;
    while (2 * L2 <= k0 - 1) L2 <<= 1;
    dbl[0][t] = rm;
    if (t < MP3D_LIM_DPAD) dbl[0][MP3D_LIM_THREADS + t] = dbl[1][MP3D_LIM_THREADS + t] = 0x7fffffff;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < L2; d <<= 1, cur ^= 1) {
        dbl[cur ^ 1][t] = min(dbl[cur][t], dbl[cur][t + d]);
        __syncthreads();
    }

    /* m[q] of indices [o0 - A, o0 + m): two spans of L cover the window of W
     * (L <= W < 2L); their running sum over the workgroup, 16 per thread,
     * modulo 2^32 (a difference of two of them is a box sum < 2^31) */
    const int nM = m + A;
    unsigned ps[MP3D_LIM_PSEG], own = 0;
    if (t * MP3D_LIM_PSEG < nM) { /* (then every run read below lies inside ra[]: run t + k0 + 1 <= NR / 16) */
        const int *const r_own = ra + t * MP3D_TP_PAD, *const r_end = ra + (t + k0) * MP3D_TP_PAD;
        const int whole = min(dbl[cur][t + 1], dbl[cur][t + k0 - L2]); /* runs t + 1 .. t + k0 - 1 */
        int sfx[MP3D_LIM_PSEG], run = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < MP3D_LIM_PSEG; u++) {
            sfx[u] = r_own[u];
            const int v = r_end[u];
            run = u < p0 ? min(run, v) : run; /* R[16 (t + k0) .. + p0) */
        }
#pragma unroll
        for (int u = MP3D_LIM_PSEG - 2; u >= 0; u--) sfx[u] = min(sfx[u], sfx[u + 1]);
        /* (runs past the last R hold whatever: the windows of q < nM end before them) */
#pragma unroll
        for (int u = 0; u < MP3D_LIM_PSEG; u++) {
            const int e = p0 + u; /* the window's last index, counted from run t + k0's first */
            run = min(run, r_end[e + (e >> 4)]);
            const int q = t * MP3D_LIM_PSEG + u;
            own += q < nM ? (unsigned)min(sfx[u], min(whole, run)) : 0u;
            ps[u] = own;
        }
    } else {
#pragma unroll
        for (int u = 0; u < MP3D_LIM_PSEG; u++) ps[u] = 0u;
    }
    unsigned incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        incl += (t & 63) >= d ? up : 0u;
    }
    if ((t & 63) == 63) wtot[t >> 6] = incl;
    __syncthreads(); /* every read of the minima is before the sums' stores */
    unsigned before = incl - own;
    for (int v = 0; v < (t >> 6); v++) before += wtot[v];
#pragma unroll
    for (int u = 0; u < MP3D_LIM_PSEG; u++) {
        const int q = t * MP3D_LIM_PSEG + u;
        if (q < nM) ra[RA(q)] = (int)(before + ps[u]);
    }
    __syncthreads();

    /* index o0 + f: the box over m[f .. f + A] of the tile's minima */
    typedef LimOut<C, F32> O;
    typename O::T *o = (typename O::T *)out + (size_t)s * (size_t)out_stride + (size_t)tile * MP3D_LIM_TILE;
    const unsigned box = (unsigned)(A + 1);
    float gmin = 1.0f;
    for (int f = t; f < m; f += MP3D_LIM_THREADS) {
        const unsigned S = (unsigned)ra[RA(f + A)] - (f ? (unsigned)ra[RA(f - 1)] : 0u);
        const float g = (float)(S / box) * (1.0f / 1048576.0f);
        const int j = f + MP3D_LIM_BACK(A);
        o[f] = O::of(sx + ((j >> 4) * MP3D_TP_PAD + (j & 15)) * C, g);
        gmin = fminf(gmin, g);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) gmin = fminf(gmin, __shfl_xor(gmin, d)); /* (a minimum: any order) */
    if ((t & 63) == 0) wmin[t >> 6] = gmin;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int v = 1; v < MP3D_LIM_WAVES; v++) gmin = fminf(gmin, wmin[v]);
        tilemin[(size_t)s * tiles + tile] = gmin;
    }
}

/* the call's smallest gain and the state after it */
template <int C>
__global__ void __launch_bounds__(MP3D_LIM_THREADS)
k_lim_carry(const float *__restrict__ samples, LimState *st, const LimPlan *__restrict__ plan,
            const float *__restrict__ gain, const float *__restrict__ tilemin, float *__restrict__ gr,
            long long sample_stride, int tiles, int A) {
    __shared__ float sc[MP3D_LIM_CARRY * C];
    __shared__ float wmin[MP3D_LIM_WAVES];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x;
    const LimPlan P = plan[s];
    LimState *S = st + s;
    if (gr) {
        float g = 1.0f;
        for (int i = t; i < P.tiles; i += MP3D_LIM_THREADS) g = fminf(g, tilemin[(size_t)s * tiles + i]);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) g = fminf(g, __shfl_xor(g, d));
        if ((t & 63) == 0) wmin[t >> 6] = g;
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int v = 1; v < MP3D_LIM_WAVES; v++) g = fminf(g, wmin[v]);
            gr[s] = g;
        }
    }
    if (P.restart) {
        if (t == 0) S->n = 0;
        return;
    }
    if (P.n_in == 0) return;
    /* the last 4A + 11 frames of v seen: the call's, before them the old carry's */
    const LimSrc<C> X(samples + (size_t)s * (size_t)sample_stride * C, S->carry, gain, s, P, A);
    const int ne = X.K * C;
    X.each(P.n_in - X.K, ne, t, [&](int e, float v) { sc[e] = v; });
    __syncthreads(); /* every read of the old carry is before the new one's stores */
    for (int e = t; e < ne; e += MP3D_LIM_THREADS) S->carry[e] = sc[e];
    if (t == 0) S->n = P.n0 + P.n_in;
}

void launch_limiter(const float *samples, const int32_t *counts, LimState *st, LimPlan *plan, const float *taps,
                    const float *gain, void *out, int32_t *out_count, float *tilemin, float *gr, bool f32, int ch, int n,
                    long long sample_stride, long long out_stride, int tiles, int A, float c, int flush,
                    hipStream_t strm) {
    const dim3 blk(MP3D_LIM_THREADS), grid((unsigned)n * (unsigned)tiles);
    hipLaunchKernelGGL(k_lim_plan, dim3((n + MP3D_LIM_THREADS - 1) / MP3D_LIM_THREADS), blk, 0, strm, st, counts, plan,
                       out_count, n, sample_stride, out_stride, A, flush);
#define MP3D_LIM_GO(C, F)                                                                                              \
    hipLaunchKernelGGL((k_lim_tile<C, F>), grid, blk, 0, strm, samples, st, plan, taps, gain, out, tilemin,            \
                       sample_stride, out_stride, tiles, A, c)
    if (ch == 2) {
        if (f32) MP3D_LIM_GO(2, true);
        else MP3D_LIM_GO(2, false);
        hipLaunchKernelGGL(k_lim_carry<2>, dim3(n), blk, 0, strm, samples, st, plan, gain, tilemin, gr, sample_stride,
                           tiles, A);
    } else {
        if (f32) MP3D_LIM_GO(1, true);
        else MP3D_LIM_GO(1, false);
        hipLaunchKernelGGL(k_lim_carry<1>, dim3(n), blk, 0, strm, samples, st, plan, gain, tilemin, gr, sample_stride,
                           tiles, A);
    }
#undef MP3D_LIM_GO
}

} // namespace mp3d
