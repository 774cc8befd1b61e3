/*
 * mp3d_segment.hip -- the segment sink: where speech starts and ends in packed
 * float32 samples, as sample ranges (include/mp3d.h "segment sink"; DESIGN.md
 * section 4i; mp3d_segment.h has the kernel list and the layouts).
 *
 * After one float32 quantisation everything is integer arithmetic, so the
 * result has one value whatever call, tile or lane computes it:
 *   q[i]   = the packed sink's int16 of the mono mix (pcm_i16)
 *   E[b]   = sum_{n < H} q[bH + n]^2                          (uint64, exact)
 *   a[b]   = E[b] >= thr
 *   c      = a with the gaps shorter than P filled: d[b] = OR_{k<P} a[b - k],
 *            c[b] = AND_{k<P} d[b + k] (a closing by P hops)
 *   o      = c without the runs shorter than S: e[t] = AND_{k<S} c[t + k],
 *            o[b] = OR_{k<S} e[b - k] (an opening by S hops)
 * The closing is the header's c: with i the last active hop <= b and j the
 * first >= b, every window of P hops from [b - P + 1, b] on holds i or j iff
 * j - i <= P.
 *
 * Mapping: k_sg_energy gives a wave a hop at a time, 16 hops per wave and 64
 * per block; its lanes read float4 (two stereo or four mono frames) from the
 * first 16-byte aligned address of the hop on, the frames before and after it
 * one per lane.  k_sg_emit keeps 4096 hops as one bit each, a 64-bit word per
 * lane: a sliding OR over n hops is log2(n) + 1 shifts of the whole set, a
 * shift is two lane shuffles and a funnel.
 */
#include "mp3d_device.h"
#include "mp3d_segment.h"
#include "mp3d_launch.h"

/* the wglds build and the product build must round alike: no contraction */
#pragma clang fp contract(off)

namespace mp3d {

static_assert(MP3D_SG_TILE == 64, "a tile's activity bits are one 64-bit word");
static_assert(MP3D_SG_THREADS % 64 == 0 && MP3D_SG_TILE % (MP3D_SG_THREADS / 64) == 0, "whole waves, each with its share of a tile");
static_assert(MP3D_SG_HOPS_PER_WAVE * (MP3D_SG_THREADS / 64) == 64 && MP3D_SG_HOPS_PER_WAVE <= 32, "a wave's bits fit a word of wbits");
static_assert(MP3D_SG_HIST >= 4 * MP3D_SG_MAXHOPS, "the history holds 2 (S + P) hops");
static_assert(MP3D_SG_CHUNK == 64 * 64 && MP3D_SG_CHUNK > 4 * MP3D_SG_MAXHOPS, "a word per lane; a chunk decides hops");
static_assert(MP3D_SG_HWORDS <= 64, "a lane per history word");
static_assert((unsigned long long)MP3D_SG_HMAX << 30 < 1ull << 63, "a hop's energy fits");

__global__ void __launch_bounds__(MP3D_SG_THREADS)
k_sg_plan(const SgState *__restrict__ st, const int32_t *__restrict__ counts, SgPlan *__restrict__ plan,
          unsigned long long *__restrict__ part, int n, long long sample_stride, int H, int flush) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_SG_THREADS + threadIdx.x;
    if (s >= n) return;
    long long c = counts[s];
    c = c < 0 ? 0 : c > sample_stride ? sample_stride : c;
    SgPlan P;
    P.n0 = st[s].n;
    P.hop0 = P.n0 / H;
    P.r0 = (int32_t)(P.n0 - P.hop0 * H);
    P.n_in = (int32_t)c;
    /* the samples of the hops from the open one on; a flush completes the last with zeros */
    const long long have = P.r0 + c, touched = (have + H - 1) / H;
    P.touched = (int32_t)touched;
    P.done = (int32_t)(flush ? touched : have / H);
    P.tiles = (int32_t)((touched + MP3D_SG_TILE - 1) / MP3D_SG_TILE);
    P.pad_ = 0;
    plan[s] = P;
    part[s] = 0; /* no hop is open after the call unless k_sg_energy finds one */
}

/* q^2 of one sample frame */
template <int C> __device__ __forceinline__ unsigned sg_sq(float x0, float x1) {
    const float m = C == 2 ? 0.5f * (x0 + x1) : x0;
    const int q = pcm_i16(m);
    return (unsigned)(q * q); /* <= 2^30 */
}

/* This lane's share of the energy of the nf sample frames from p on.  p is
 * float-aligned; 16-byte loads from the first aligned address on, the frames
 * before and after them one per lane (at most three each). */
template <int C> __device__ __forceinline__ unsigned long long sg_span(const float *p, int nf, int lane) {
    unsigned long long acc = 0;
    if (C == 2 && ((uintptr_t)p & 4)) { /* rows that start half a frame off 8 bytes: no aligned load holds whole frames */
        for (int i = lane; i < nf; i += 64) acc += sg_sq<2>(p[2 * i], p[2 * i + 1]);
        return acc;
    }
    const int ne = nf * C;
    const int head = min((int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2), ne); /* whole frames: p is frame-aligned */
    if (lane * C < head) acc += sg_sq<C>(p[lane * C], C == 2 ? p[lane * C + 1] : 0.0f);
    const float4 *v = (const float4 *)(p + head);
    const int nv = (ne - head) >> 2;
    for (int i = lane; i < nv; i += 64) {
        const float4 x = v[i];
        if (C == 2) {
            acc += sg_sq<2>(x.x, x.y);
            acc += sg_sq<2>(x.z, x.w);
        } else {
            acc += sg_sq<1>(x.x, 0.0f);
            acc += sg_sq<1>(x.y, 0.0f);
            acc += sg_sq<1>(x.z, 0.0f);
            acc += sg_sq<1>(x.w, 0.0f);
        }
    }
    const int at = head + 4 * nv + lane * C;
    if (at < ne) acc += sg_sq<C>(p[at], C == 2 ? p[at + 1] : 0.0f);
    return acc;
}

template <int C>
__global__ void __launch_bounds__(MP3D_SG_THREADS)
k_sg_energy(const float *__restrict__ samples, const SgState *__restrict__ st, const SgPlan *__restrict__ plan,
            const unsigned long long *__restrict__ thr, unsigned long long *__restrict__ part,
            unsigned long long *__restrict__ bits, long long sample_stride, int n, int tiles, int H) {
    __shared__ unsigned wbits[MP3D_SG_THREADS / 64];
    MP3D_LDS_ENTRY();
    /* Tile-major: workgroups go to the eight XCDs in turn, so with the streams innermost every XCD gets its
     * share of each tile index; stream-major, a tile index (the full first tile, the part one behind it, the
     * empty ones of a stride sized for the worst case) would land on the same XCDs for every stream. */
    const int s = blockIdx.x % n, tile = blockIdx.x / n, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const SgPlan P = plan[s];
    if (tile >= P.tiles) return;
    const float *row = samples + (size_t)s * (size_t)sample_stride * C;
    const unsigned long long th = thr[s];
    unsigned mine = 0;
    for (int i = 0; i < MP3D_SG_HOPS_PER_WAVE; i++) {
        /* hop k of the call, counted from the open one: the call's samples [k H - r0, (k + 1) H - r0) */
        const int k = tile * MP3D_SG_TILE + w * MP3D_SG_HOPS_PER_WAVE + i;
        if (k >= P.touched) break;
        const long long lo = max((long long)k * H - P.r0, 0LL), hi = min((long long)(k + 1) * H - P.r0, (long long)P.n_in);
        unsigned long long e = sg_span<C>(row + lo * C, (int)(hi - lo), lane);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) e += __shfl_xor(e, d); /* (integers: any order) */
        if (k == 0) e += st[s].epart;
        if (k < P.done) mine |= (unsigned)(e >= th) << i;
        else if (lane == 0) part[s] = e; /* the one hop the call leaves open */
    }
    if (lane == 0) wbits[w] = mine;
    __syncthreads();
    if (t == 0) {
        unsigned long long word = 0;
#pragma unroll
        for (int v = 0; v < MP3D_SG_THREADS / 64; v++) word |= (unsigned long long)wbits[v] << (v * MP3D_SG_HOPS_PER_WAVE);
        bits[(size_t)s * tiles + tile] = word;
    }
}

/* the chunk's 4096 bits moved k places up (towards later hops) or down, zeros moving in; 0 <= k < 4096 - 64 */
template <bool DOWN> __device__ __forceinline__ unsigned long long sg_shift(unsigned long long x, int k, int lane) {
    const int ws = k >> 6, bs = k & 63;
    unsigned long long a, b;
    if (DOWN) {
        a = __shfl_down(x, ws), b = __shfl_down(x, ws + 1);
        a = lane + ws < 64 ? a : 0, b = lane + ws + 1 < 64 ? b : 0;
        return bs ? (a >> bs) | (b << (64 - bs)) : a;
    }
    a = __shfl_up(x, ws), b = __shfl_up(x, ws + 1);
    a = lane >= ws ? a : 0, b = lane >= ws + 1 ? b : 0;
    return bs ? (a << bs) | (b >> (64 - bs)) : a;
}

/* OR over a window of n >= 1 places: bit b of the result is the OR of x[b - k] (up) or x[b + k] (DOWN), k < n:
 * doubling to the largest power of two m <= n, then two windows of m that cover n */
template <bool DOWN> __device__ __forceinline__ unsigned long long sg_winor(unsigned long long x, int n, int lane) {
    int m = 1;
    for (; 2 * m <= n; m *= 2) x |= sg_shift<DOWN>(x, m, lane);
    if (n > m) x |= sg_shift<DOWN>(x, n - m, lane);
    return x;
}

/* bits [x0, x1) of a word, both clipped to it */
__device__ __forceinline__ unsigned long long sg_range(int x0, int x1) {
    x0 = max(x0, 0), x1 = min(x1, 64);
    if (x1 <= x0) return 0;
    const unsigned long long upto = x1 == 64 ? ~0ull : (1ull << x1) - 1;
    return upto & ~((1ull << x0) - 1);
}

__global__ void __launch_bounds__(64)
k_sg_emit(SgState *st, const SgPlan *__restrict__ plan, const unsigned long long *__restrict__ part,
          const unsigned long long *__restrict__ bits, long long *__restrict__ seg, int32_t *__restrict__ seg_count,
          long long seg_stride, int tiles, int H, int Pp, int S, int pad, int flush) {
    __shared__ unsigned long long sh[MP3D_SG_HWORDS];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, lane = threadIdx.x;
    const SgPlan P = plan[s];
    SgState *Z = st + s;
    if (lane < MP3D_SG_HWORDS) sh[lane] = Z->hist[lane];
    __syncthreads();
    const unsigned long long *cw = bits + (size_t)s * tiles;
    /* The hops as one bit string: the history a[B0 - 1024 .. B0), the call's
     * `done` bits, zeros from there on.  64 bits of it from place v >= 0 on. */
    auto word = [&](long long j) -> unsigned long long {
        if (j < MP3D_SG_HWORDS) return sh[j];
        return j - MP3D_SG_HWORDS < P.tiles ? cw[j - MP3D_SG_HWORDS] : 0ull;
    };
    auto bits64 = [&](long long v) -> unsigned long long {
        const long long j = v >> 6;
        const int r = (int)(v & 63);
        const unsigned long long lo = word(j) >> r;
        return r ? lo | word(j + 1) << (64 - r) : lo;
    };
    const int W = S + Pp, OUT = MP3D_SG_CHUNK - 2 * W;
    const long long B0 = P.hop0, B1 = B0 + P.done, N1 = P.n0 + P.n_in;
    /* o[b] is final for b <= B - W: [D0, D1) is what this call decides; a flush decides o[B] = 0 too */
    const long long D0 = max(B0 - W + 1, 0LL), D1 = flush ? B1 + 1 : max(B1 - W + 1, 0LL);
    int total = 0;
    long long last = Z->b0;
    /* the first pass counts, the second writes: a slot that overflows writes nothing */
    for (int pass = 0; pass < 2; pass++) {
        int idx = 0;
        last = Z->b0;
        for (long long lo = D0; lo < D1; lo += OUT) {
            /* the chunk: hops [base, base + 4096), of which [lo, hi) are decided here;
             * W hops below them and at least W above are in it */
            const long long hi = min(lo + OUT, D1), base = lo - W;
            const unsigned long long a = bits64(base - (B0 - MP3D_SG_HIST) + 64 * lane);
            const unsigned long long d = sg_winor<false>(a, Pp, lane);
            const unsigned long long c = ~sg_winor<true>(~d, Pp, lane);
            const unsigned long long e = ~sg_winor<true>(~c, S, lane);
            const unsigned long long o = sg_winor<false>(e, S, lane);
            /* (what moves in at the chunk's ends spoils W - 2 hops at each: none of [lo - 1, hi)) */
            const unsigned long long prev = sg_shift<false>(o, 1, lane);
            const unsigned long long m = sg_range(W - 64 * lane, W + (int)(hi - lo) - 64 * lane);
            const unsigned long long rise = o & ~prev & m, fall = ~o & prev & m;
            const long long hop = base + 64 * lane; /* of the word's bit 0 */
            const int cnt = __popcll(fall);
            int inc = cnt;
            long long sc = rise ? hop + 63 - __clzll(rise) : -1; /* the last rising edge up to this lane */
#pragma unroll
            for (int dl = 1; dl < 64; dl <<= 1) {
                const int ui = __shfl_up(inc, dl);
                const long long us = __shfl_up(sc, dl);
                if (lane >= dl) inc += ui, sc = max(sc, us);
            }
            if (pass) {
                long long before = __shfl_up(sc, 1);
                before = lane ? max(before, last) : last;
                int k = idx + inc - cnt;
                for (unsigned long long f = fall; f; f &= f - 1, k++) {
                    const int p = __ffsll((long long)f) - 1;
                    const unsigned long long below = rise & ((1ull << p) - 1);
                    const long long b0 = below ? hop + 63 - __clzll(below) : before, b1 = hop + p;
                    long long *out = seg + ((size_t)s * (size_t)seg_stride + (size_t)k) * 2;
                    out[0] = max(b0 - pad, 0LL) * H;
                    out[1] = min((b1 + pad) * H, N1); /* (the min acts at a flush only: b1 + pad < B otherwise) */
                }
            }
            idx += __shfl(inc, 63);
            last = max(last, __shfl(sc, 63));
        }
        total = idx;
        if (total > seg_stride) break;
    }
    const bool over = total > seg_stride;
    if (lane == 0) seg_count[s] = over ? -1 : total;
    if (flush || over) { /* the slot restarts */
        if (lane < MP3D_SG_HWORDS) Z->hist[lane] = 0;
        if (lane == 0) Z->n = 0, Z->epart = 0, Z->b0 = 0;
        return;
    }
    /* (the history is read from sh, never from the state it replaces) */
    if (lane < MP3D_SG_HWORDS) Z->hist[lane] = bits64((long long)P.done + 64 * lane);
    if (lane == 0) Z->n = N1, Z->epart = part[s], Z->b0 = last;
}

void launch_segments(const float *samples, const int32_t *counts, SgState *st, SgPlan *plan, const uint64_t *thr,
                     uint64_t *part, uint64_t *bits, long long *seg, int32_t *seg_count, int ch, int n,
                     long long sample_stride, long long seg_stride, int tiles, int H, int P, int S, int pad, int flush,
                     hipStream_t strm) {
    typedef unsigned long long u64;
    const dim3 blk(MP3D_SG_THREADS), grid((unsigned)n * (unsigned)tiles);
    hipLaunchKernelGGL(k_sg_plan, dim3((n + MP3D_SG_THREADS - 1) / MP3D_SG_THREADS), blk, 0, strm, st, counts, plan,
                       (u64 *)part, n, sample_stride, H, flush);
    if (ch == 2)
        hipLaunchKernelGGL(k_sg_energy<2>, grid, blk, 0, strm, samples, st, plan, (const u64 *)thr, (u64 *)part,
                           (u64 *)bits, sample_stride, n, tiles, H);
    else
        hipLaunchKernelGGL(k_sg_energy<1>, grid, blk, 0, strm, samples, st, plan, (const u64 *)thr, (u64 *)part,
                           (u64 *)bits, sample_stride, n, tiles, H);
    hipLaunchKernelGGL(k_sg_emit, dim3(n), dim3(64), 0, strm, st, plan, (const u64 *)part, (const u64 *)bits, seg,
                       seg_count, seg_stride, tiles, H, P, S, pad, flush);
}

} // namespace mp3d
