/*
 * mp3d_pitch.hip -- the pitch sink: the fundamental frequency of packed
 * float32 samples per 10 ms hop by YIN (include/mp3d.h "pitch sink";
 * DESIGN.md section 4k; mp3d_pitch.h has the kernel list, the order of the
 * kernels and the layouts).
 *
 * After one float32 quantisation everything up to the record's two floats is
 * integer arithmetic, so a record has one value whatever call, tile or lane
 * computes it:
 *   q[i]   = the packed sink's int16 of the mono mix (pcm_i16)
 *   r[i]   = q[f H + i] >> sh, |r| <= 1024                  (block floating point)
 *   D(tau) = Q[W] + (Q[tau + W] - Q[tau]) - 2 X(tau)        (< 2^32, exact)
 *   S(tau) = sum_{k <= tau} D(k)                            (uint64, exact)
 * and the floats are single IEEE double operations on exact integers, rounded
 * once to float32.
 */
#include "mp3d_device.h"
#include "mp3d_pitch.h"
#include "mp3d_launch.h"

/* the wglds build and the product build must round alike: no contraction */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_PT_THREADS == 256, "four waves: their partial results are joined through arrays of four");
static_assert(MP3D_PT_LAGS == 4, "a window of eight words: four held, four read");
static_assert(MP3D_PT_ROW % 8 == 0 && (MP3D_PT_ROW / 2) % 64 == 32, "16-byte rows of int16, 32 banks apart mod 64");
static_assert(2 * (MP3D_PT_TMAX / 8 + 1) <= MP3D_PT_THREADS, "a thread per parity and group of eight lags");
/* uint4 index (ck + 1) + g of a copy: ck < ceil(HMAX / 4), g <= TMAX / 8 */
static_assert(4 * ((MP3D_PT_HMAX + 3) / 4 + 1 + MP3D_PT_TMAX / 8) + 4 <= MP3D_PT_ROW / 2, "every thread's reads stay inside a row");
static_assert(MP3D_PT_ROW >= 8 * MP3D_PT_THREADS && MP3D_PT_SPANMAX <= 8 * MP3D_PT_THREADS, "eight squares per thread cover a frame");
static_assert(4 * MP3D_PT_THREADS >= MP3D_PT_TMAX, "four lags of D per thread cover the range");
static_assert((long long)MP3D_PT_SPANMAX << 20 < 1LL << 31, "Q fits 31 bits");

typedef short s16x2 __attribute__((ext_vector_type(2)));

#define PT_NONE 0x7fffffff

/* frames known after N samples */
__device__ __forceinline__ long long pt_known(long long N, int H, int SPAN) { return N < SPAN ? 0 : (N - SPAN) / H + 1; }

/* q of sample frame i of a row: the tempo sink's mono mix, the packed sink's int16 */
template <int C> __device__ __forceinline__ short pt_q(const float *row, long long i) {
    float m = row[i * C];
    if (C == 2) m = 0.5f * (m + row[i * C + 1]);
    return pcm_i16(m);
}

__global__ void __launch_bounds__(MP3D_PT_THREADS)
k_pt_plan(const PtState *__restrict__ st, const int32_t *__restrict__ counts, PtPlan *__restrict__ plan,
          int32_t *__restrict__ out_count, int n, long long sample_stride, long long pitch_stride, int H, int SPAN,
          int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_PT_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    PtPlan P;
    P.n0 = st[s].n;
    P.f0 = pt_known(P.n0, H, SPAN);
    P.n_in = (int32_t)c;
    const long long n1 = P.n0 + c;
    /* a flush emits every frame that starts inside the stream */
    const long long f1 = flush ? (n1 + H - 1) / H : pt_known(n1, H, SPAN), emit = f1 - P.f0;
    const bool over = emit > pitch_stride;
    P.emit = over ? 0 : (int32_t)emit;
    P.tiles = (P.emit + MP3D_PT_TILE - 1) / MP3D_PT_TILE;
    P.restart = flush || over;
    plan[s] = P;
    out_count[s] = over ? -1 : (int32_t)emit;
}

__device__ __forceinline__ int pt_wave_min(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}

template <int C>
__global__ void __launch_bounds__(MP3D_PT_THREADS)
k_pt_frames(const float *__restrict__ samples, const PtState *__restrict__ st, const PtPlan *__restrict__ plan,
            uint32_t *__restrict__ rec, long long sample_stride, long long pitch_stride, int n, int fs, int H, int T,
            int tmin, int theta) {
    __shared__ __attribute__((aligned(16))) short stg[MP3D_PT_STAGE];
    __shared__ __attribute__((aligned(16))) short qc[2][MP3D_PT_ROW];
    __shared__ __attribute__((aligned(16))) short rf[2 * MP3D_PT_HMAX + 16];
    __shared__ unsigned Qp[8 * MP3D_PT_THREADS + 4];
    __shared__ unsigned Dl[4 * MP3D_PT_THREADS + 4];
    __shared__ int xs[MP3D_PT_THREADS * MP3D_PT_LAGS];
    __shared__ unsigned long long wS[4];
    __shared__ unsigned wq[4];
    __shared__ int wmx[4], wt0[4], wt1[4];
    MP3D_LDS_ENTRY();
    /* tile-major, as k_sg_energy: every XCD gets its share of each tile index */
    const int s = blockIdx.x % n, tile = blockIdx.x / n, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const PtPlan P = plan[s];
    if (tile >= P.tiles) return;
    const int W = 2 * H, SPAN = W + T, tmax = T - 1;
    const int nf = min(MP3D_PT_TILE, P.emit - tile * MP3D_PT_TILE);
    const float *row = samples + (size_t)s * (size_t)sample_stride * C;
    const short *carry = st[s].carry;
    /* the stream's samples by their index since the restart: [c0, n0) from the carry, [n0, n1) from the call,
     * zeros elsewhere (before the carry there is nothing a frame of this call reads: mp3d.h) */
    const long long n0 = P.n0, c0 = n0 - min(n0, (long long)SPAN - 1), n1 = n0 + P.n_in;
    const long long g0 = (P.f0 + (long long)tile * MP3D_PT_TILE) * H;
    const int len = (nf - 1) * H + SPAN;
    for (int i = t; i < len; i += MP3D_PT_THREADS) {
        const long long g = g0 + i;
        short v = 0;
        if (g >= n0) {
            if (g < n1) v = pt_q<C>(row, g - n0);
        } else if (g >= c0) v = carry[g - c0];
        stg[i] = v;
    }
    __syncthreads();

    /* the lags' threads: parity p and group g of u own lags 8 g + p + 2 k; the sample pairs in NS segments */
    const int nt = 2 * (T / 8 + 1), NS = MP3D_PT_THREADS / nt, seg = t / nt, u = t - seg * nt;
    const int nck = (H + 3) / 4; /* W / 2 = H pairs, four to a read */
    const int ck0 = seg < NS ? seg * nck / NS : 0, ck1 = seg < NS ? (seg + 1) * nck / NS : 0;

    for (int fi = 0; fi < nf; fi++) {
        const short *x = stg + fi * H;
        /* 1. block floating point */
        int mx = 0;
        for (int i = t; i < SPAN; i += MP3D_PT_THREADS) mx = max(mx, abs((int)x[i]));
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
        if (lane == 0) wmx[w] = mx;
        __syncthreads();
        mx = max(max(wmx[0], wmx[1]), max(wmx[2], wmx[3]));
        const int sh = max(0, 32 - __clz(mx) - 10);
        for (int i = t; i < MP3D_PT_ROW; i += MP3D_PT_THREADS) {
            const short v = i < SPAN ? (short)(x[i] >> sh) : (short)0;
            qc[0][i] = v;
            if (i) qc[1][i - 1] = v;
            if (i < 2 * MP3D_PT_HMAX + 16) rf[i] = i < W ? v : (short)0;
        }
        if (t == 0) qc[1][MP3D_PT_ROW - 1] = 0;
        __syncthreads();
        /* 2. Q: the running sum of the squares, eight per thread */
        unsigned sq[8], own = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int v = qc[0][8 * t + k];
            own += (unsigned)(v * v);
            sq[k] = own;
        }
        unsigned incl = own;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned up = __shfl_up(incl, m);
            incl += lane >= m ? up : 0u;
        }
        if (lane == 63) wq[w] = incl;
        /* 3. X: sixteen dot products per two 16-byte reads */
        if (seg < NS) {
            const int par = u & 1, g = u >> 1;
            const uint4 *pc = (const uint4 *)qc[par] + g, *pr = (const uint4 *)rf;
            int xa[MP3D_PT_LAGS] = {0, 0, 0, 0};
            uint4 cur = pc[ck0];
            for (int ck = ck0; ck < ck1; ck++) {
                const uint4 nxt = pc[ck + 1], rr = pr[ck];
                const uint32_t win[8] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z, nxt.w};
                const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int k = 0; k < MP3D_PT_LAGS; k++)
                        xa[k] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, rw[j]),
                                                       __builtin_bit_cast(s16x2, win[j + k]), xa[k], false);
                cur = nxt;
            }
#pragma unroll
            for (int k = 0; k < MP3D_PT_LAGS; k++) xs[t * MP3D_PT_LAGS + k] = xa[k];
        }
        __syncthreads();
        {
            unsigned base = incl - own;
            for (int v = 0; v < w; v++) base += wq[v];
            if (t == 0) Qp[0] = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) Qp[8 * t + k + 1] = base + sq[k];
        }
        __syncthreads();
        /* 4. D and S of lags 4 t + 1 .. 4 t + 4 */
        unsigned d[4];
        unsigned long long sc[4], acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int tau = 4 * t + 1 + k;
            d[k] = 0;
            if (tau <= T) {
                const int lu = 2 * (tau >> 3) + (tau & 1), lk = (tau & 7) >> 1;
                long long X = 0;
                for (int v = 0; v < NS; v++) X += xs[(v * nt + lu) * MP3D_PT_LAGS + lk];
                d[k] = (unsigned)((long long)Qp[W] + ((long long)Qp[tau + W] - (long long)Qp[tau]) - 2 * X);
            }
            Dl[tau] = d[k];
            acc += d[k];
            sc[k] = acc;
        }
        unsigned long long inc2 = acc;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long up = __shfl_up(inc2, m);
            inc2 += lane >= m ? up : 0ull;
        }
        if (lane == 63) wS[w] = inc2;
        __syncthreads();
        unsigned long long sbase = inc2 - acc;
        for (int v = 0; v < w; v++) sbase += wS[v];
        /* 5. t0: the smallest lag under the threshold */
        int cand = PT_NONE;
#pragma unroll
        for (int k = 3; k >= 0; k--) {
            const int tau = 4 * t + 1 + k;
            if (tau >= tmin && tau <= tmax &&
                (unsigned long long)d[k] * (unsigned long long)(tau * 1024) < (unsigned long long)theta * (sbase + sc[k]))
                cand = tau;
        }
        cand = pt_wave_min(cand);
        if (lane == 0) wt0[w] = cand;
        __syncthreads();
        const int t0 = min(min(wt0[0], wt0[1]), min(wt0[2], wt0[3]));
        /* 6. the walk to the local minimum of D: the first lag from t0 on that does not fall */
        cand = PT_NONE;
#pragma unroll
        for (int k = 3; k >= 0; k--) {
            const int tau = 4 * t + 1 + k;
            if (tau >= t0 && tau <= tmax && (tau == tmax || Dl[tau + 1] >= d[k])) cand = tau;
        }
        cand = pt_wave_min(cand);
        if (lane == 0) wt1[w] = cand;
        __syncthreads();
        const int tt = min(min(wt1[0], wt1[1]), min(wt1[2], wt1[3]));
        uint32_t *o = rec + ((size_t)s * (size_t)pitch_stride + (size_t)(tile * MP3D_PT_TILE + fi)) * 4;
        if (t0 == PT_NONE) {
            if (t == 0) o[0] = 0, o[1] = 0, o[2] = 0, o[3] = (uint32_t)sh;
        } else if (t == (tt - 1) >> 2) {
            /* 7. the parabola and the record, by the thread that holds S(tt) */
            const int k = (tt - 1) & 3;
            const long long a = Dl[tt - 1], b = Dl[tt], c = Dl[tt + 1];
            const unsigned long long St = sbase + (k == 0 ? sc[0] : k == 1 ? sc[1] : k == 2 ? sc[2] : sc[3]);
            const long long den = a - 2 * b + c;
            double delta = 0.0;
            if (den > 0) {
                const double hn = 0.5 * (double)(a - c);
                delta = hn / (double)den;
            }
            delta = delta < -1.0 ? -1.0 : delta > 1.0 ? 1.0 : delta;
            const double lagf = (double)tt + delta;
            const float f0 = (float)((double)fs / lagf);
            const double ratio = (double)(b * tt) / (double)St;
            const double per = 1.0 - ratio;
            const float pf = (float)(per > 0.0 ? per : 0.0);
            o[0] = __float_as_uint(f0), o[1] = __float_as_uint(pf), o[2] = (uint32_t)tt, o[3] = (uint32_t)sh;
        }
        /* (the next frame's first stores to wmx, qc, rf, Qp, xs, Dl and the w* arrays come after barriers that
         * follow this frame's last reads of each) */
    }
}

template <int C>
__global__ void __launch_bounds__(MP3D_PT_THREADS)
k_pt_update(const float *__restrict__ samples, PtState *st, const PtPlan *__restrict__ plan, long long sample_stride,
            int SPAN) {
    __shared__ short nc[MP3D_PT_CARRY + 1];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x;
    const PtPlan P = plan[s];
    PtState *Z = st + s;
    if (P.restart) {
        if (t == 0) Z->n = 0;
        return;
    }
    if (P.n_in == 0) return;
    const float *row = samples + (size_t)s * (size_t)sample_stride * C;
    const long long n0 = P.n0, c0 = n0 - min(n0, (long long)SPAN - 1), n1 = n0 + P.n_in;
    const int keep = (int)min(n1, (long long)SPAN - 1);
    const long long c1 = n1 - keep; /* c1 >= c0 */
    for (int i = t; i < keep; i += MP3D_PT_THREADS) {
        const long long g = c1 + i;
        nc[i] = g < n0 ? Z->carry[g - c0] : pt_q<C>(row, g - n0);
    }
    __syncthreads(); /* every read of the old carry is before the new one's stores */
    for (int i = t; i < keep; i += MP3D_PT_THREADS) Z->carry[i] = nc[i];
    if (t == 0) Z->n = n1;
}

void launch_pitch(const float *samples, const int32_t *counts, PtState *st, PtPlan *plan, void *rec,
                  int32_t *rec_count, int ch, int n, long long sample_stride, long long pitch_stride, int tiles, int fs,
                  int H, int T, int tmin, int theta, int flush, hipStream_t strm) {
    const dim3 blk(MP3D_PT_THREADS), grid((unsigned)n * (unsigned)tiles);
    const int SPAN = 2 * H + T;
    hipLaunchKernelGGL(k_pt_plan, dim3((n + MP3D_PT_THREADS - 1) / MP3D_PT_THREADS), blk, 0, strm, st, counts, plan,
                       rec_count, n, sample_stride, pitch_stride, H, SPAN, flush);
    if (ch == 2) {
        hipLaunchKernelGGL(k_pt_frames<2>, grid, blk, 0, strm, samples, st, plan, (uint32_t *)rec, sample_stride,
                           pitch_stride, n, fs, H, T, tmin, theta);
        hipLaunchKernelGGL(k_pt_update<2>, dim3(n), blk, 0, strm, samples, st, plan, sample_stride, SPAN);
    } else {
        hipLaunchKernelGGL(k_pt_frames<1>, grid, blk, 0, strm, samples, st, plan, (uint32_t *)rec, sample_stride,
                           pitch_stride, n, fs, H, T, tmin, theta);
        hipLaunchKernelGGL(k_pt_update<1>, dim3(n), blk, 0, strm, samples, st, plan, sample_stride, SPAN);
    }
}

} // namespace mp3d
