/*
 * mp3d_resample.hip -- the packed uniform-rate PCM sink: channel map and
 * polyphase resampling of a call's float32 rows into contiguous samples per
 * stream at one rate and channel count ("Packed PCM sink").
 *
 * Output m of a stream is  y[m] = sum_j taps[p][j] * x[n0 - pre + j],
 * n0 = floor(m M / L), p = (m M) mod L, accumulated by ONE float32 FMA chain
 * in ascending j whatever thread, tile or call computes it; inputs before the
 * stream start, and after its end in a flushed call, are staged as zeros so
 * the chain has the same length everywhere.
 *
 * Mapping (k_rs_filter): one 256-thread block per (stream, output tile).  The
 * block stages the tile's input span -- history, then the rows' samples with
 * the channel map applied, interleaved by output channel -- into LDS.
 *  - Upsampling (48 taps per phase, up to 1 280 phases, the phases of
 *    consecutive outputs scattered over the table): a thread walks outputs
 *    m, m + S, m + 2S ... with S a multiple of L, so its phase never changes
 *    and its 48 taps are loaded into registers once per pass (S / 256 passes
 *    per tile, each load serving tile / S outputs: 3 to 4 at 44.1 -> 48 kHz,
 *    DESIGN.md section 4b); lanes hold consecutive
 *    m, so their LDS reads are (nearly) consecutive and their stores coalesce.
 *  - Downsampling (54 .. 288 taps): a thread walks m, m + 256 ...; the taps
 *    come from the table (at most 87 KB per rate pair, L2 / L1 resident) in
 *    16-byte loads of its phase's row, 4 FMAs per channel for each.
 *  - Equal rates: the staged samples are copied.
 * A stream's sample window (RsState lo, hi, r: a gapless trim from its tag or
 * an explicit crop) is applied while staging: k_rs_plan turns it into the
 * call's skip and kept count, and the filter and the update read kept sample
 * rel at sample rel + skip of the prefix.
 * These inner loops are rs_tile, shared with the long-stream sink below
 * (k_rsl_plan / k_rsl_filter / k_rsl_carry, mp3d_batch_decode_long_packed):
 * one stream, staged chunk by chunk straight from the segments' rows, with
 * the gapless trim applied while staging.
 */
#include "mp3d_device.h"
#include "mp3d_resample.h"
#include "mp3d_launch.h"

namespace mp3d {

__device__ __forceinline__ int rs_rate_index(int hz) {
    const int R[MP3D_RS_RATES] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000};
    int k = -1;
#pragma unroll
    for (int i = 0; i < MP3D_RS_RATES; i++) k = hz == R[i] ? i : k;
    return k;
}

__device__ __forceinline__ long long rs_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

/* outputs emitted once n inputs were seen: those with n0 + post <= n - 1 */
__device__ __forceinline__ long long rs_emitted(long long n, const RsFilt &f) {
    return n > f.post ? rs_ceil_div((n - f.post) * f.L, f.M) : 0;
}

/* The gapless window of a stream from its tag words (StreamState tag_info,
 * tag_frames, kind): tag_to_info (mp3d_batch.cpp), FFmpeg's skip and end of
 * the LAME tag.  [0, no end) without the flag or a LAME / Lavf / Lavc tag. */
__device__ __forceinline__ void rs_tag_window(const uint32_t *__restrict__ tag, int gapless, long long &lo, long long &hi) {
    lo = 0;
    hi = INT64_MAX;
    const uint32_t tg = tag[0];
    if (gapless && (tg & MP3D_TAG_LAME)) {
        lo = (long long)((tg >> 12) & 0xFFFu) + 529;
        const int frames = (tg & MP3D_TAG_FRAMES) ? (int)tag[1] : -1;
        if (frames > 0) {
            const long long end = (long long)frames * ((int)tag[2] == 2 ? 576 : 1152) + 529 - (long long)(tg & 0xFFFu);
            if (end >= 0) hi = end;
        }
    }
}

/* st[s]'s window is written here (fixed by the first call that feeds the slot
 * a sample), the rest of the state by k_rs_update */
__global__ void __launch_bounds__(MP3D_RS_THREADS)
k_rs_plan(const DevInfo *__restrict__ inf, RsState *__restrict__ st, const StreamState *__restrict__ sst,
          const RsCfg *__restrict__ cfg, RsPlan *__restrict__ plan, int32_t *__restrict__ prefix,
          int32_t *__restrict__ out_count, int n, int F, long long stride, int flush, int gapless) {
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x * MP3D_RS_THREADS + threadIdx.x;
    if (s >= n) return;
    int ri = st[s].rate_i;
    const long long pos = ri ? st[s].pos : 0;
    int nin = 0;
    int32_t *pf = prefix + (size_t)s * (F + 1);
    for (int f = 0; f < F; f++) {
        const DevInfo d = inf[(size_t)s * F + f];
        pf[f] = nin;
        if (d.samples > 0 && d.samples <= 1152 && (d.channels == 1 || d.channels == 2)) {
            if (!ri) ri = rs_rate_index(d.hz) + 1;
            if (ri) nin += d.samples;
        }
    }
    pf[F] = nin;
    /* the window: samples [a, b) of the call's nin are kept */
    long long lo = 0, hi = INT64_MAX;
    if (st[s].fixed) {
        lo = st[s].lo;
        hi = st[s].hi;
    } else if (nin > 0) {
        rs_tag_window(&sst[s].tag_info, gapless, lo, hi);
        st[s].fixed = 1;
        st[s].lo = lo;
        st[s].hi = hi;
    }
    const long long r = st[s].r;
    const int a = (int)min(max(lo - r, 0LL), (long long)nin);
    const int b = (int)min(max(hi - r, (long long)a), (long long)nin);
    RsPlan P;
    P.pos = pos;
    P.m0 = 0;
    P.rate_i = ri;
    P.n_in = b - a;
    P.count = 0;
    P.restart = flush;
    P.skip = a;
    P.fed = nin;
    if (ri) {
        const RsFilt f = cfg->f[ri - 1];
        const long long n1 = pos + P.n_in;
        P.m0 = rs_emitted(pos, f);
        const long long m1 = flush ? rs_ceil_div(n1 * f.L, f.M) : rs_emitted(n1, f);
        const long long c = m1 - P.m0;
        if (c > stride) {
            P.count = -1;
            P.restart = 1;
        } else {
            P.count = (int)c;
        }
    }
    plan[s] = P;
    out_count[s] = P.count;
}

/* sample k of a row with ch channels, mapped to OC channels */
template <int OC>
__device__ __forceinline__ void rs_load(const float *__restrict__ row, int ch, int k, float *v) {
    if (ch == 2) {
        const float2 a = *(const float2 *)(row + 2 * k);
        if (OC == 2) {
            v[0] = a.x;
            v[1] = a.y;
        } else {
            v[0] = 0.5f * (a.x + a.y);
        }
    } else {
        const float a = row[k];
        v[0] = a;
        if (OC == 2) v[1] = a;
    }
}

/* the frame holding input sample rel (0 <= rel < prefix[F]): the last f with
 * prefix[f] <= rel */
__device__ __forceinline__ int rs_frame_of(const int32_t *__restrict__ pf, int F, int rel) {
    int lo = 0, hi = F; /* prefix[lo] <= rel < prefix[hi] */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pf[mid] <= rel) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <int OC, bool F32>
__device__ __forceinline__ void rs_store(void *__restrict__ out, size_t at, const float *acc) {
    if (F32) {
        if (OC == 2) *(float2 *)((float *)out + at) = make_float2(acc[0], acc[1]);
        else ((float *)out)[at] = acc[0];
    } else {
        short q[OC]; /* (the library's int16 rounding: mp3d_device.h) */
#pragma unroll
        for (int c = 0; c < OC; c++) q[c] = pcm_i16(acc[c]);
        if (OC == 2) *(short2 *)((short *)out + at) = make_short2(q[0], q[1]);
        else ((short *)out)[at] = q[0];
    }
}

/* The n outputs of one tile from its staged input span, by the whole block
 * (thread t): output i of the tile is output M0 + i of the stream and goes to
 * element at0 + i * OC of out; sx[0] is input X0 of the stream (M0 and X0 may
 * both be reduced by the same multiples of L and M: k_rs_filter's are). */
template <int OC, bool F32>
__device__ __forceinline__ void rs_tile(const float *__restrict__ sx, const RsFilt &f, const float *__restrict__ tab,
                                        long long M0, int n, long long X0, void *__restrict__ out, size_t at0, int t) {
    if (f.T == 1) { /* equal rates: copy */
        for (int mo = t; mo < n; mo += MP3D_RS_THREADS) {
            const int xi = (int)(M0 + mo - X0);
            float acc[OC];
#pragma unroll
            for (int c = 0; c < OC; c++) acc[c] = sx[xi * OC + c];
            rs_store<OC, F32>(out, at0 + (size_t)mo * OC, acc);
        }
        return;
    }
    const float *ft = tab + f.off;
    if (f.T == MP3D_RS_UP_TAPS) {
        /* one phase per thread and pass: f.S is a multiple of L */
        const int step = (int)((long long)f.S * f.M / f.L);
        for (int r = t; r < f.S; r += MP3D_RS_THREADS) {
            if (r >= n) break;
            const long long mm = (M0 + r) * f.M;
            const int p = (int)(mm % f.L);
            int xi = (int)(mm / f.L - f.pre - X0);
            float4 tp[MP3D_RS_UP_TAPS / 4];
#pragma unroll
            for (int j = 0; j < MP3D_RS_UP_TAPS / 4; j++) tp[j] = *(const float4 *)(ft + (size_t)p * f.Tp + 4 * j);
            for (int mo = r; mo < n; mo += f.S, xi += step) {
                float acc[OC];
#pragma unroll
                for (int c = 0; c < OC; c++) acc[c] = 0.0f;
                const float *x = sx + xi * OC;
#pragma unroll
                for (int j = 0; j < MP3D_RS_UP_TAPS / 4; j++) {
                    const float w[4] = {tp[j].x, tp[j].y, tp[j].z, tp[j].w};
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int c = 0; c < OC; c++) acc[c] = fmaf(w[q], x[(4 * j + q) * OC + c], acc[c]);
                }
                rs_store<OC, F32>(out, at0 + (size_t)mo * OC, acc);
            }
        }
        return;
    }
    /* general: consecutive outputs on consecutive threads, taps from the table */
    if (t >= n) return;
    const long long mm = (M0 + t) * f.M;
    int p = (int)(mm % f.L);
    int xi = (int)(mm / f.L - f.pre - X0);
    const int dq = (int)((long long)MP3D_RS_THREADS * f.M / f.L), dr = (int)((long long)MP3D_RS_THREADS * f.M % f.L);
    const int T4 = f.T & ~3;
    for (int mo = t; mo < n; mo += MP3D_RS_THREADS) {
        float acc[OC];
#pragma unroll
        for (int c = 0; c < OC; c++) acc[c] = 0.0f;
        const float *x = sx + xi * OC;
        const float *w = ft + (size_t)p * f.Tp;
        for (int j = 0; j < T4; j += 4) {
            const float4 w4 = *(const float4 *)(w + j);
            const float wq[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int c = 0; c < OC; c++) acc[c] = fmaf(wq[q], x[(j + q) * OC + c], acc[c]);
        }
        for (int j = T4; j < f.T; j++)
#pragma unroll
            for (int c = 0; c < OC; c++) acc[c] = fmaf(w[j], x[j * OC + c], acc[c]);
        rs_store<OC, F32>(out, at0 + (size_t)mo * OC, acc);
        xi += dq;
        p += dr;
        if (p >= f.L) {
            p -= f.L;
            xi++;
        }
    }
}

template <int OC, bool F32>
__global__ void __launch_bounds__(MP3D_RS_THREADS)
k_rs_filter(const float *__restrict__ rows, const DevInfo *__restrict__ inf, const RsState *__restrict__ st,
            const RsCfg *__restrict__ cfg, const float *__restrict__ tab, const RsPlan *__restrict__ plan,
            const int32_t *__restrict__ prefix, void *__restrict__ out, int F, long long stride, int tiles) {
    __shared__ __attribute__((aligned(16))) float sx[(MP3D_RS_SPAN + 8) * OC];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, t = threadIdx.x;
    const RsPlan P = plan[s];
    if (P.count <= 0) return;
    const RsFilt f = cfg->f[P.rate_i - 1];
    const long long mA = (long long)tile * f.tile;
    if (mA >= P.count) return;
    const int mB = (int)min((long long)P.count, mA + f.tile); /* outputs [mA, mB) of the call */
    /* input span [nA, nB) of the tile, relative to the call's first sample */
    const int relA = (int)(((P.m0 + mA) * f.M) / f.L - f.pre - P.pos);
    const int relB = (int)(((P.m0 + mB - 1) * f.M) / f.L + f.post + 1 - P.pos);
    const int len = min(relB - relA, MP3D_RS_SPAN); /* <= SPAN by the choice of f.tile */
    const int HL = f.pre + f.post;
    const float *hist = st[s].hist;
    /* history before the call's samples, zeros after them (a flushed call) */
    for (int i = t; i < len; i += MP3D_RS_THREADS) {
        const int rel = relA + i;
        if (rel >= 0 && rel < P.n_in) continue;
#pragma unroll
        for (int c = 0; c < OC; c++) sx[i * OC + c] = rel < 0 && HL + rel >= 0 ? hist[(HL + rel) * OC + c] : 0.0f;
    }
    /* kept samples [lo, hi) - skip of the call, as samples of its prefix */
    const int lo = max(relA, 0) + P.skip, hi = min(relA + len, P.n_in) + P.skip;
    if (lo < hi) {
        const int sx0 = -relA - P.skip; /* sample of the prefix -> element of sx */
        const int32_t *pf = prefix + (size_t)s * (F + 1);
        for (int fr = rs_frame_of(pf, F, lo); fr < F; fr++) {
            const int a = pf[fr], b = pf[fr + 1];
            if (a >= hi) break;
            if (b <= a) continue;
            const int ch = inf[(size_t)s * F + fr].channels;
            const float *row = rows + ((size_t)s * F + fr) * 2304;
            for (int k = max(a, lo) + t; k < min(b, hi); k += MP3D_RS_THREADS) {
                float v[OC];
                rs_load<OC>(row, ch, k - a, v);
#pragma unroll
                for (int c = 0; c < OC; c++) sx[(k + sx0) * OC + c] = v[c];
            }
        }
    }
    __syncthreads();
    rs_tile<OC, F32>(sx, f, tab, P.m0 + mA, mB - (int)mA, P.pos + relA, out,
                     ((size_t)s * (size_t)stride + (size_t)mA) * OC, t);
}

/* the state after the call: the last pre + post kept inputs, the position,
 * the fed count */
template <int OC>
__global__ void __launch_bounds__(MP3D_RS_THREADS)
k_rs_update(const float *__restrict__ rows, const DevInfo *__restrict__ inf, RsState *__restrict__ st,
            const RsCfg *__restrict__ cfg, const RsPlan *__restrict__ plan, const int32_t *__restrict__ prefix, int F) {
    __shared__ float nh[MP3D_RS_HIST * OC];
    MP3D_LDS_ENTRY();
    const int s = blockIdx.x, t = threadIdx.x;
    const RsPlan P = plan[s];
    RsState *S = st + s;
    if (P.restart) {
        for (int i = t; i < MP3D_RS_HIST * 2; i += MP3D_RS_THREADS) S->hist[i] = 0.0f;
        if (t == 0) {
            /* the resampler restarts; the window and its count carry on */
            S->rate_i = 0;
            S->pos = 0;
            S->r += P.fed;
        }
        return;
    }
    if (!P.rate_i || !P.fed) return;
    const RsFilt f = cfg->f[P.rate_i - 1];
    if (P.n_in) { /* (a call that kept nothing leaves the history as it is) */
        const int HL = f.pre + f.post;
        const int32_t *pf = prefix + (size_t)s * (F + 1);
        for (int i = t; i < HL; i += MP3D_RS_THREADS) {
            const int rel = P.n_in - HL + i;
            float v[OC];
            if (rel < 0) {
#pragma unroll
                for (int c = 0; c < OC; c++) v[c] = S->hist[(HL + rel) * OC + c];
            } else {
                const int k = rel + P.skip;
                const int fr = rs_frame_of(pf, F, k);
                rs_load<OC>(rows + ((size_t)s * F + fr) * 2304, inf[(size_t)s * F + fr].channels, k - pf[fr], v);
            }
#pragma unroll
            for (int c = 0; c < OC; c++) nh[i * OC + c] = v[c];
        }
        __syncthreads();
        for (int i = t; i < HL * OC; i += MP3D_RS_THREADS) S->hist[i] = nh[i];
    }
    if (t == 0) {
        long long pos = P.pos + P.n_in;
        if (pos >= (long long)f.post + f.M) pos = f.post + (pos - f.post) % f.M;
        S->rate_i = P.rate_i;
        S->pos = pos;
        S->r += P.fed;
    }
}

/* ------------------------------------------------------------------------ */
/* The long-stream sink (mp3d_resample.h RsLong)       */
/* ------------------------------------------------------------------------ */
/* slot in the chunk's batch output of its output frame jl: k_gather_frames'
 * indirection (a = the segments' first decoded frame, from the chunk's first) */
__device__ __forceinline__ size_t rsl_slot(const int *__restrict__ a, int L, int F, int k0, int jl) {
    const int k = jl / L;
    const int j = (k0 + k) * L + jl % L;
    return (size_t)k * F + (size_t)(j - a[k]);
}

/* a frame slot that feeds the sink (k_rs_plan's rule) */
__device__ __forceinline__ bool rsl_audio(const DevInfo &d) {
    return d.samples > 0 && d.samples <= 1152 && (d.channels == 1 || d.channels == 2);
}

/* k_rsl_plan is one block and latency-bound (a[k], then the frame's info, per
 * frame): 1 024 threads x 8 frames make a stride 8 192 frames, so a chunk of
 * 1 024 segments of 32 frames takes four */
#define MP3D_RSL_PLAN_THREADS 1024
#define MP3D_RSL_PER 8 /* frames per thread and stride of k_rsl_plan's scan */

/* trimmed inputs seen once r inputs were seen */
__device__ __forceinline__ long long rsl_trimmed(long long r, long long lo, long long hi) {
    return max(min(r, hi) - lo, 0LL);
}

__global__ void __launch_bounds__(MP3D_RSL_PLAN_THREADS)
k_rsl_plan(const DevInfo *__restrict__ inf, const int *__restrict__ a, const uint32_t *__restrict__ tag,
           const RsCfg *__restrict__ cfg, RsLong *__restrict__ S, int32_t *__restrict__ prefix, int L, int F, int k0,
           int n_out, int first, int last, int gapless) {
    __shared__ int32_t wsum[MP3D_RSL_PLAN_THREADS / 64];
    __shared__ int32_t s_base, s_first;
    MP3D_LDS_ENTRY();
    const int t = threadIdx.x;
    if (t == 0) {
        s_base = 0;
        s_first = n_out;
    }
    __syncthreads();
    /* the input rate: the stream's first audio frame (in the first stride of
     * the first chunk, unless the stream opens with that many empty slots) */
    const int ri0 = S->rate_i;
    int ri = ri0;
    if (!ri) {
        for (int j0 = 0; j0 < n_out; j0 += MP3D_RSL_PLAN_THREADS) {
            const int jl = j0 + t;
            bool hit = false;
            if (jl < n_out) {
                const DevInfo d = inf[rsl_slot(a, L, F, k0, jl)];
                hit = rsl_audio(d) && rs_rate_index(d.hz) >= 0;
            }
            if (hit) atomicMin(&s_first, jl);
            if (__syncthreads_or(hit)) break;
        }
        if (s_first < n_out) ri = rs_rate_index(inf[rsl_slot(a, L, F, k0, s_first)].hz) + 1;
    }
    const int from = ri0 ? 0 : s_first; /* frames before the rate is known feed nothing */
    /* exclusive prefix sum: PER consecutive frames per thread, a wave scan of
     * the threads' sums, the waves' totals through LDS, the running base */
    for (int j0 = 0; j0 < n_out; j0 += MP3D_RSL_PLAN_THREADS * MP3D_RSL_PER) {
        const int jb = j0 + t * MP3D_RSL_PER;
        int v[MP3D_RSL_PER], sum = 0;
#pragma unroll
        for (int i = 0; i < MP3D_RSL_PER; i++) {
            const int jl = jb + i;
            v[i] = 0;
            if (jl < n_out && jl >= from) {
                const DevInfo d = inf[rsl_slot(a, L, F, k0, jl)];
                if (rsl_audio(d)) v[i] = d.samples;
            }
            sum += v[i];
        }
        int inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if ((t & 63) >= o) inc += u;
        }
        if ((t & 63) == 63) wsum[t >> 6] = inc;
        __syncthreads();
        int before = s_base;
        for (int w = 0; w < (t >> 6); w++) before += wsum[w];
        int run = before + inc - sum;
#pragma unroll
        for (int i = 0; i < MP3D_RSL_PER; i++) {
            if (jb + i < n_out) prefix[jb + i] = run;
            run += v[i];
        }
        __syncthreads();
        if (t == MP3D_RSL_PLAN_THREADS - 1) s_base = before + inc;
        __syncthreads();
    }
    if (t != 0) return;
    const int n_in = s_base;
    prefix[n_out] = n_in;
    long long lo = S->lo, hi = S->hi;
    if (first) {
        rs_tag_window(tag, gapless, lo, hi);
        S->lo = lo;
        S->hi = hi;
    }
    const long long r0 = S->raw, m0 = S->m1;
    const long long q0 = rsl_trimmed(r0, lo, hi), q1 = rsl_trimmed(r0 + n_in, lo, hi);
    long long m1 = m0;
    if (ri) {
        const RsFilt f = cfg->f[ri - 1];
        m1 = last ? rs_ceil_div(q1 * f.L, f.M) : rs_emitted(q1, f);
    }
    S->rate_i = ri;
    S->n_in = n_in;
    S->q0 = q0;
    S->q1 = q1;
    S->m0 = m0;
    S->m1 = max(m1, m0);
}

template <int OC, bool F32>
__global__ void __launch_bounds__(MP3D_RS_THREADS)
k_rsl_filter(const float *__restrict__ rows, const DevInfo *__restrict__ inf, const int *__restrict__ a,
             const RsCfg *__restrict__ cfg, const float *__restrict__ tab, const RsLong *__restrict__ S,
             const int32_t *__restrict__ prefix, void *__restrict__ out, long long cap, int L, int F, int k0, int n_out) {
    __shared__ __attribute__((aligned(16))) float sx[(MP3D_RS_SPAN + 8) * OC];
    MP3D_LDS_ENTRY();
    const int t = threadIdx.x;
    const long long mEnd = min((long long)S->m1, cap); /* nothing at or past the caller's capacity is written */
    if (!S->rate_i || S->m0 >= mEnd) return;
    const RsFilt f = cfg->f[S->rate_i - 1];
    const long long mA = S->m0 + (long long)blockIdx.x * f.tile;
    if (mA >= mEnd) return;
    const long long mB = min(mEnd, mA + f.tile); /* outputs [mA, mB) of the stream */
    /* trimmed inputs [qA, qA + len) of the tile */
    const long long qA = (mA * f.M) / f.L - f.pre;
    const long long qB = ((mB - 1) * f.M) / f.L + f.post + 1;
    const int len = (int)min(qB - qA, (long long)MP3D_RS_SPAN); /* <= SPAN by the choice of f.tile */
    const int HL = f.pre + f.post;
    const long long q0 = S->q0, q1 = S->q1;
    /* the carry before the chunk's samples; zeros before the stream's first
     * sample and, in the last chunk, after its last */
    for (int i = t; i < len; i += MP3D_RS_THREADS) {
        const long long q = qA + i;
        if (q >= q0 && q < q1) continue;
        const long long h = q - (q0 - HL);
        const bool old = q >= 0 && q < q0 && h >= 0;
#pragma unroll
        for (int c = 0; c < OC; c++) sx[i * OC + c] = old ? S->hist[h * OC + c] : 0.0f;
    }
    const long long qlo = max(qA, q0), qhi = min(qA + len, q1);
    if (qlo < qhi) {
        /* q -> sample of the chunk, before the trim */
        const long long shift = S->lo - S->raw;
        const int lo = (int)(qlo + shift), hi = (int)(qhi + shift);
        const int sx0 = (int)(qlo - qA) - lo;
        for (int fr = rs_frame_of(prefix, n_out, lo); fr < n_out; fr++) {
            const int pa = prefix[fr], pb = prefix[fr + 1];
            if (pa >= hi) break;
            if (pb <= pa) continue;
            const size_t sf = rsl_slot(a, L, F, k0, fr);
            const int ch = inf[sf].channels;
            const float *row = rows + sf * 2304;
            for (int k = max(pa, lo) + t; k < min(pb, hi); k += MP3D_RS_THREADS) {
                float v[OC];
                rs_load<OC>(row, ch, k - pa, v);
#pragma unroll
                for (int c = 0; c < OC; c++) sx[(k + sx0) * OC + c] = v[c];
            }
        }
    }
    __syncthreads();
    rs_tile<OC, F32>(sx, f, tab, mA, (int)(mB - mA), qA, out, (size_t)mA * OC, t);
}

/* the carry after the chunk: the last T - 1 trimmed inputs (from the old
 * carry where the chunk holds fewer), the input count */
template <int OC>
__global__ void __launch_bounds__(MP3D_RS_THREADS)
k_rsl_carry(const float *__restrict__ rows, const DevInfo *__restrict__ inf, const int *__restrict__ a,
            const RsCfg *__restrict__ cfg, RsLong *__restrict__ S, const int32_t *__restrict__ prefix, int L, int F,
            int k0, int n_out) {
    __shared__ float nh[MP3D_RS_HIST * OC];
    MP3D_LDS_ENTRY();
    const int t = threadIdx.x;
    const long long q0 = S->q0, q1 = S->q1, r0 = S->raw;
    const int n_in = S->n_in;
    if (S->rate_i && q1 > q0) {
        const RsFilt f = cfg->f[S->rate_i - 1];
        const int HL = f.pre + f.post;
        const long long shift = S->lo - r0;
        for (int i = t; i < HL; i += MP3D_RS_THREADS) {
            const long long q = q1 - HL + i;
            float v[OC];
#pragma unroll
            for (int c = 0; c < OC; c++) v[c] = 0.0f;
            if (q >= q0) {
                const int rel = (int)(q + shift);
                const int fr = rs_frame_of(prefix, n_out, rel);
                const size_t sf = rsl_slot(a, L, F, k0, fr);
                rs_load<OC>(rows + sf * 2304, inf[sf].channels, rel - prefix[fr], v);
            } else if (q >= 0 && q - (q0 - HL) >= 0) {
#pragma unroll
                for (int c = 0; c < OC; c++) v[c] = S->hist[(q - (q0 - HL)) * OC + c];
            }
#pragma unroll
            for (int c = 0; c < OC; c++) nh[i * OC + c] = v[c];
        }
        __syncthreads();
        for (int i = t; i < HL * OC; i += MP3D_RS_THREADS) S->hist[i] = nh[i];
    }
    if (t == 0) S->raw = r0 + n_in;
}

void launch_resample_long(const float *rows, const void *infos, const int *a, const uint32_t *tag, const RsCfg *cfg,
                          int out_ch, const float *tab, RsLong *st, int32_t *prefix, void *out, bool f32, long long cap,
                          int L, int F, int k0, int n_out, int tiles, int first, int last, int gapless, hipStream_t strm) {
    const DevInfo *inf = (const DevInfo *)infos;
    const dim3 blk(MP3D_RS_THREADS);
    hipLaunchKernelGGL(k_rsl_plan, dim3(1), dim3(MP3D_RSL_PLAN_THREADS), 0, strm, inf, a, tag, cfg, st, prefix, L, F, k0,
                       n_out, first, last, gapless);
#define RSL_FILTER(OC, F32)                                                                                            \
    hipLaunchKernelGGL((k_rsl_filter<OC, F32>), dim3((unsigned)tiles), blk, 0, strm, rows, inf, a, cfg, tab, st, prefix, \
                       out, cap, L, F, k0, n_out)
    if (out_ch == 2) {
        if (f32) RSL_FILTER(2, true);
        else RSL_FILTER(2, false);
        hipLaunchKernelGGL(k_rsl_carry<2>, dim3(1), blk, 0, strm, rows, inf, a, cfg, st, prefix, L, F, k0, n_out);
    } else {
        if (f32) RSL_FILTER(1, true);
        else RSL_FILTER(1, false);
        hipLaunchKernelGGL(k_rsl_carry<1>, dim3(1), blk, 0, strm, rows, inf, a, cfg, st, prefix, L, F, k0, n_out);
    }
#undef RSL_FILTER
}

void launch_resample(const float *rows, const void *infos, RsState *st, const StreamState *sst, const RsCfg *cfg,
                     int out_ch, const float *tab, RsPlan *plan, int32_t *prefix, void *out, bool f32,
                     int32_t *out_count, int n, int F, long long stride, int tiles, int flush, int gapless,
                     hipStream_t strm) {
    const DevInfo *inf = (const DevInfo *)infos;
    hipLaunchKernelGGL(k_rs_plan, dim3((n + MP3D_RS_THREADS - 1) / MP3D_RS_THREADS), dim3(MP3D_RS_THREADS), 0, strm, inf,
                       st, sst, cfg, plan, prefix, out_count, n, F, stride, flush, gapless);
    const dim3 grid((unsigned)n * (unsigned)tiles), blk(MP3D_RS_THREADS);
#define RS_FILTER(OC, F32)                                                                                             \
    hipLaunchKernelGGL((k_rs_filter<OC, F32>), grid, blk, 0, strm, rows, inf, st, cfg, tab, plan, prefix, out, F, stride, \
                       tiles)
    if (out_ch == 2) {
        if (f32) RS_FILTER(2, true);
        else RS_FILTER(2, false);
    } else {
        if (f32) RS_FILTER(1, true);
        else RS_FILTER(1, false);
    }
#undef RS_FILTER
    if (out_ch == 2)
        hipLaunchKernelGGL(k_rs_update<2>, dim3(n), blk, 0, strm, rows, inf, st, cfg, plan, prefix, F);
    else
        hipLaunchKernelGGL(k_rs_update<1>, dim3(n), blk, 0, strm, rows, inf, st, cfg, plan, prefix, F);
}

} // namespace mp3d
