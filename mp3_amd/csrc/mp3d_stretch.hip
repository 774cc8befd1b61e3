/*
 * mp3d_stretch.hip -- the tempo sink: a pitch-preserving time stretch (WSOLA)
 * of packed float32 samples (include/mp3d.h "tempo sink"; DESIGN.md section
 * 4g; mp3d_stretch.h has the kernel list and the layouts).
 *
 * Every value is exact integer arithmetic or one float32 rounding, so the
 * output has one value whatever call or lane computes it:
 *   q[i]   = clamp(floor(m[i] * 1024 + 0.5), -1023, 1023), m the mono mix
 *   d(dl)  = sum_n (q[r + n] - q[t + dl + n])^2              (int32, exact)
 *   y[n]   = x[r + n] + fl(w[n] * fl(x[a + n] - x[r + n]))   (not fused)
 *
 * Mapping (k_st_blocks): one 256-thread block per stream walks the stream's
 * blocks in order.  A block's H reference samples and H + 2D candidate-span
 * samples are staged into LDS as int16; the span twice, the second copy one
 * sample ahead, so a candidate ci reads 32-bit pairs at word (ci >> 1) + j of
 * copy (ci & 1) whatever its parity.  The search expands
 *   d(ci) = E_ref + E(ci) - 2 X(ci),  E(ci) = sum_n c[ci + n]^2,
 *   X(ci) = sum_n q_ref[n] c[ci + n]
 * and drops E_ref, which is the same for every candidate.  Thread t owns the
 * candidates 4 (t / 2) + (t & 1) and that + 2: the same parity, one word
 * apart, so each span word it reads serves both, one packed int16 dot product
 * (v_dot2 on gfx950) per candidate and pair of samples against the broadcast
 * reference pair.  The lanes of a wave read every second word of a copy, and
 * the copies lie an odd number of words apart: even lanes on even banks, odd
 * lanes on odd ones.  E comes from one running sum of the span's squares
 * over the workgroup (four per thread, a wave scan, the waves' totals through
 * LDS).  The minimum is one signed 64-bit key (d * 1024 + |delta| * 2 +
 * (delta > 0)), reduced by wave shuffles and a four-entry LDS array.
 */
#include "mp3d_device.h"
#include "mp3d_stretch.h"
#include "mp3d_launch.h"

/* three separately rounded operations per output sample, in both builds */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_ST_THREADS == 256, "four waves: their keys are joined through wkey[4]");
static_assert(2 * MP3D_ST_QMAX * 2 * MP3D_ST_QMAX * (long long)MP3D_ST_HMAX < 0x7fffffffLL, "d fits int32");
static_assert(MP3D_ST_DMAX < 512, "|delta| is 9 bits of the key");
/* the second copy of the span starts an odd number of banks after the first */
#define MP3D_ST_QROW 1090
static_assert(MP3D_ST_QROW % 2 == 0 && (MP3D_ST_QROW / 2) % 2 == 1, "rows of int16, an odd number of banks apart");
/* thread t reads words 2 (t / 2) .. 2 (t / 2) + (H + 1) / 2 of its copy */
static_assert(MP3D_ST_QROW >= 2 * MP3D_ST_THREADS + MP3D_ST_HMAX + 2 && MP3D_ST_QROW >= MP3D_ST_SPAN + 2,
              "every thread's reads stay inside a row");
static_assert(MP3D_ST_SPAN * MP3D_ST_QMAX * (long long)MP3D_ST_QMAX < 0x7fffffffLL, "the span's energy fits int32");

typedef short s16x2 __attribute__((ext_vector_type(2)));

/* t_k = floor(k H num / den), k >= 0 */
__device__ __forceinline__ long long st_t(long long k, int H, int num, int den) { return k * H * num / den; }

/* block k is emitted once sample e_k has been seen */
__device__ __forceinline__ long long st_e(long long k, int H, int num, int den) {
    const long long tk = st_t(k, H, num, den), tp = k ? st_t(k - 1, H, num, den) : -(long long)H;
    return max(max(tk, tp + H) + H / 2 + H - 1, st_t(k + 1, H, num, den) - 1);
}

__global__ void __launch_bounds__(MP3D_ST_THREADS)
k_st_plan(const StState *__restrict__ st, const int32_t *__restrict__ tempo, const int32_t *__restrict__ counts,
          StPlan *__restrict__ plan, int32_t *__restrict__ out_count, int n, long long sample_stride,
          long long out_stride, int H, int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_ST_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    const int num = tempo[2 * s], den = tempo[2 * s + 1];
    const long long k0 = st[s].k, n1 = st[s].n + c;
    long long blocks, n_out;
    if (flush) {
        /* every block under M = ceil(N den / num), the last one cut to M */
        const long long M = (n1 * den + num - 1) / num;
        n_out = max(0LL, M - k0 * H);
        blocks = (n_out + H - 1) / H;
    } else {
        /* e_k does not fall with k: the first k >= k0 with e_k > N - 1, by
         * bisection; t_hi > N already, so hi is never emitted */
        long long lo = k0, hi = max(k0, (n1 + 1) * den / ((long long)num * H) + 1);
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (st_e(mid, H, num, den) <= n1 - 1) lo = mid + 1;
            else hi = mid;
        }
        blocks = lo - k0;
        n_out = blocks * H;
    }
    const bool over = n_out > out_stride;
    StPlan P;
    P.n_in = (int32_t)c;
    P.blocks = over ? 0 : (int32_t)blocks;
    P.n_out = over ? -1 : (int32_t)n_out;
    P.restart = flush || over;
    plan[s] = P;
    out_count[s] = P.n_out;
}

/* The stream's samples by their index since the restart: [c0, n0) from the
 * carry, [n0, n1) from the call, zeros elsewhere (past a flushed end). */
template <int C> struct StSrc {
    const float *row, *carry;
    long long c0, n0, n1;
    __device__ __forceinline__ float at(long long i, int c) const {
        if (i < c0 || i >= n1) return 0.0f;
        return i < n0 ? carry[(i - c0) * C + c] : row[(i - n0) * C + c];
    }
    /* the match signal: 11 bits of the mono mix */
    __device__ __forceinline__ short q(long long i) const {
        float m = at(i, 0);
        if (C == 2) m = 0.5f * (m + at(i, 1));
        const float v = floorf(m * 1024.0f + 0.5f);
        return (short)fminf(fmaxf(v, -(float)MP3D_ST_QMAX), (float)MP3D_ST_QMAX); /* (a NaN becomes -1023) */
    }
};

template <int C>
__global__ void __launch_bounds__(MP3D_ST_THREADS)
k_st_blocks(const float *__restrict__ samples, StState *st, const int32_t *__restrict__ tempo,
            const StPlan *__restrict__ plan, const float *__restrict__ w, float *__restrict__ out,
            long long sample_stride, long long out_stride, int H) {
    __shared__ __attribute__((aligned(16))) short qr[MP3D_ST_HMAX + 2];
    __shared__ __attribute__((aligned(16))) short qc[2][MP3D_ST_QROW];
    __shared__ int pre[MP3D_ST_SPAN + 4], wtot[MP3D_ST_THREADS / 64];
    __shared__ long long wkey[MP3D_ST_THREADS / 64];
    __shared__ float sc[MP3D_ST_CARRY * C];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x, D = H / 2;
    const StPlan P = plan[s];
    StState *S = st + s;
    if (P.restart && P.blocks == 0) { /* an overflow, or a flush with nothing pending */
        if (t == 0) S->n = S->k = S->r = S->c0 = 0;
        return;
    }
    const int num = tempo[2 * s], den = tempo[2 * s + 1];
    StSrc<C> X;
    X.row = samples + (size_t)s * (size_t)sample_stride * C;
    X.carry = S->carry;
    X.n0 = S->n;
    X.c0 = max(S->c0, X.n0 - MP3D_ST_CARRY); /* (the carry never holds more: mp3d_stretch.h) */
    X.n1 = X.n0 + P.n_in;
    long long k = S->k, r = S->r;
    float *o = out + (size_t)s * (size_t)out_stride * C;

    for (int j = 0; j < P.blocks; j++, k++) {
        const long long tk = st_t(k, H, num, den);
        long long a = 0; /* a_0 = 0 */
        if (k > 0) {
            const long long lo = tk - D; /* candidate ci starts at lo + ci */
            const int L = H + 2 * D, HP = (H + 1) / 2;
            for (int i = t; i < H; i += MP3D_ST_THREADS) qr[i] = X.q(r + i);
            if (t < 2) qr[H + t] = 0; /* an odd H's last pair is (q[H - 1], 0) */
            for (int i = t; i < L; i += MP3D_ST_THREADS) {
                const short v = X.q(lo + i);
                qc[0][i] = v;
                if (i) qc[1][i - 1] = v;
            }
            __syncthreads();
            /* E: the span's squares, four per thread, as a running sum over the workgroup */
            int sq[4], own = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int v = 4 * t + u < L ? (int)qc[0][4 * t + u] : 0;
                own += v * v;
                sq[u] = own;
            }
            int incl = own;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const int up = __shfl_up(incl, m);
                incl += (t & 63) >= m ? up : 0;
            }
            if ((t & 63) == 63) wtot[t >> 6] = incl;
            /* X: both candidates' cross terms with the reference, each span word read once */
            const int par = t & 1, g = t >> 1;
            const uint32_t *pr = (const uint32_t *)qr, *pc = (const uint32_t *)qc[par] + 2 * g;
            int xa = 0, xb = 0;
            uint32_t cur = pc[0];
#pragma unroll 8
            for (int p = 0; p < HP; p++) {
                const uint32_t nxt = pc[p + 1];
                const s16x2 rr = __builtin_bit_cast(s16x2, pr[p]);
                xa = __builtin_amdgcn_sdot2(rr, __builtin_bit_cast(s16x2, cur), xa, false);
                xb = __builtin_amdgcn_sdot2(rr, __builtin_bit_cast(s16x2, nxt), xb, false);
                cur = nxt;
            }
            __syncthreads();
            int base = incl - own;
            for (int v = 0; v < (t >> 6); v++) base += wtot[v];
            if (t == 0) pre[0] = 0;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (4 * t + u < L) pre[4 * t + u + 1] = base + sq[u];
            __syncthreads();
            long long best = 0x7fffffffffffffffLL;
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int ci = 4 * g + par + 2 * u, delta = ci - D;
                if (ci > 2 * D || lo + ci < 0) continue; /* t_k + delta >= 0 */
                const int d = pre[ci + H] - pre[ci] - 2 * (u ? xb : xa); /* d_k(delta) - E_ref */
                const long long key = (long long)d * 1024 + ((delta < 0 ? -delta : delta) << 1) + (delta > 0 ? 1 : 0);
                best = key < best ? key : best;
            }
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                const long long other = __shfl_xor(best, m);
                best = other < best ? other : best;
            }
            if ((t & 63) == 0) wkey[t >> 6] = best;
            __syncthreads();
#pragma unroll
            for (int v = 0; v < MP3D_ST_THREADS / 64; v++) best = wkey[v] < best ? wkey[v] : best;
            const int ad = (int)(best & 1023) >> 1;
            a = tk + ((best & 1) ? ad : -ad); /* (delta = 0 is always a candidate) */
        }
        /* the block's samples: the continuation of the last segment faded into the best match */
        const int len = (int)min((long long)H, (long long)P.n_out - (long long)j * H);
        for (int e = t; e < len * C; e += MP3D_ST_THREADS) {
            const int n = e / C, c = e - n * C;
            const float xr = X.at(r + n, c), xa = X.at(a + n, c);
            const float df = xa - xr;
            const float pf = w[n] * df;
            o[(size_t)j * H * C + e] = xr + pf;
        }
        r = a + H;
        __syncthreads(); /* qr, qc, pre, wtot and wkey are rewritten by the next block */
    }

    if (P.restart) {
        if (t == 0) S->n = S->k = S->r = S->c0 = 0;
        return;
    }
    if (P.n_in == 0 && P.blocks == 0) return;
    /* the carry of the next block k: from max(0, min(r_k, t_k - D)) on (r_k <= N) */
    long long c1 = max(0LL, min(r, st_t(k, H, num, den) - D));
    c1 = min(max(c1, X.n1 - MP3D_ST_CARRY), X.n1);
    const int ne = (int)(X.n1 - c1) * C;
    for (int e = t; e < ne; e += MP3D_ST_THREADS) sc[e] = X.at(c1 + e / C, e % C);
    __syncthreads(); /* every read of the old carry is before the new one's stores */
    for (int e = t; e < ne; e += MP3D_ST_THREADS) S->carry[e] = sc[e];
    if (t == 0) {
        S->n = X.n1;
        S->k = k;
        S->r = r;
        S->c0 = c1;
    }
}

void launch_stretch(const float *samples, const int32_t *counts, StState *st, const int32_t *tempo, StPlan *plan,
                    const float *w, float *out, int32_t *out_count, int n, long long sample_stride,
                    long long out_stride, int H, int ch, int flush, hipStream_t strm) {
    const dim3 blk(MP3D_ST_THREADS);
    hipLaunchKernelGGL(k_st_plan, dim3((n + MP3D_ST_THREADS - 1) / MP3D_ST_THREADS), blk, 0, strm, st, tempo, counts,
                       plan, out_count, n, sample_stride, out_stride, H, flush);
    if (ch == 2)
        hipLaunchKernelGGL(k_st_blocks<2>, dim3(n), blk, 0, strm, samples, st, tempo, plan, w, out, sample_stride,
                           out_stride, H);
    else
        hipLaunchKernelGGL(k_st_blocks<1>, dim3(n), blk, 0, strm, samples, st, tempo, plan, w, out, sample_stride,
                           out_stride, H);
}

} // namespace mp3d
