/*
 * mp3d_loudness.cpp -- the loudness sink on top of the packed sink: the
 * K-weighting design and its state-transition tables, the gated integrated
 * loudness on the host, and the calls around mp3d_loudness.hip
 * (include/mp3d.h "loudness sink").
 */
#include "mp3d_host.h"

#include <memory>

using namespace mp3d;

static int ld_block(int hz) { return (hz + 5) / 10; }

/* the two biquads of include/mp3d.h for fs = hz: b0 b1 b2 a1 a2 per stage */
static void ld_design(int hz, double *c) {
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(M_PI * f0 / hz), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(M_PI * f0 / hz), a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0;
        c[6] = -2.0;
        c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

extern "C" long long mp3d_loudness_filter(int hz, double *coef, size_t cap) {
    if (rs_rate_index(hz) < 0) return MP3D_E_ARG;
    if (coef) {
        if (cap < 10) return MP3D_E_ARG;
        ld_design(hz, coef);
    }
    return 10;
}

extern "C" long long mp3d_loud_max_blocks(int out_hz, int frames, int min_in_hz) {
    const long long S = mp3d_packed_max_samples(out_hz, frames, min_in_hz);
    if (S <= 0) return S;
    const int H = ld_block(out_hz);
    return (H - 1 + S) / H;
}

extern "C" int mp3d_loudness_integrated(const float *z, long long n, double *lufs) {
    if (!lufs || n < 0 || (n && !z)) return MP3D_E_ARG;
    *lufs = -HUGE_VAL;
    if (n < 4) return MP3D_OK;
    const long long m = n - 3;
    auto G = [z](long long j) { return ((double)z[j] + (double)z[j + 1] + (double)z[j + 2] + (double)z[j + 3]) / 4.0; };
    double s1 = 0.0, s2 = 0.0;
    long long c1 = 0, c2 = 0;
    for (long long j = 0; j < m; j++)
        if (-0.691 + 10.0 * log10(G(j)) > -70.0) s1 += G(j), c1++;
    if (!c1) return MP3D_OK;
    const double gamma = -0.691 + 10.0 * log10(s1 / (double)c1) - 10.0;
    for (long long j = 0; j < m; j++) {
        const double l = -0.691 + 10.0 * log10(G(j));
        if (l > -70.0 && l > gamma) s2 += G(j), c2++;
    }
    if (c2) *lufs = -0.691 + 10.0 * log10(s2 / (double)c2);
    return MP3D_OK;
}

/* The cascade's state transition for a zero input, A[r][j] (the kernels'
 * ld_step with v = 0), and its powers A^(SEG t) and A^(TILE t), in long double. */
typedef long double ld_mat[4][4];
static void ld_mul(const ld_mat a, const ld_mat b, ld_mat out) {
    ld_mat r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            long double acc = 0;
            for (int k = 0; k < 4; k++) acc += a[i][k] * b[k][j];
            r[i][j] = acc;
        }
    memcpy(out, r, sizeof(r));
}
static void ld_build(int hz, int ch, LdTab &t) {
    memset(&t, 0, sizeof(t));
    ld_design(hz, t.coef);
    const double *c = t.coef;
    ld_mat A;
    for (int j = 0; j < 4; j++) {
        long double s[4] = {0, 0, 0, 0};
        s[j] = 1;
        const long double o1 = s[0], o2 = (long double)c[5] * o1 + s[2];
        A[0][j] = -(long double)c[3] * o1 + s[1];
        A[1][j] = -(long double)c[4] * o1;
        A[2][j] = (long double)c[6] * o1 - (long double)c[8] * o2 + s[3];
        A[3][j] = (long double)c[7] * o1 - (long double)c[9] * o2;
    }
    ld_mat seg, p;
    memcpy(seg, A, sizeof(seg));
    static_assert(MP3D_LD_SEG == 16, "A^SEG by four squarings");
    for (int i = 0; i < 4; i++) ld_mul(seg, seg, seg);
    memset(p, 0, sizeof(p));
    for (int i = 0; i < 4; i++) p[i][i] = 1;
    for (int k = 0; k <= MP3D_LD_THREADS; k++) {
        if (k <= 64)
            for (int i = 0; i < 16; i++) t.apow[k][i] = (double)p[i / 4][i % 4];
        if (k < MP3D_LD_THREADS) ld_mul(p, seg, p);
    }
    ld_mat tile, q; /* p = A^(SEG THREADS) = A^TILE */
    memcpy(tile, p, sizeof(tile));
    memset(q, 0, sizeof(q));
    for (int i = 0; i < 4; i++) q[i][i] = 1;
    for (int k = 0; k <= 64; k++) {
        for (int i = 0; i < 16; i++) t.tpow[k][i] = (double)q[i / 4][i % 4];
        ld_mul(q, tile, q);
    }
    t.H = ld_block(hz);
    t.ch = ch;
}

extern "C" int mp3d_batch_set_loudness(mp3d_batch *b, int on) {
    if (!b || (on && !b->rs.f.hz)) return MP3D_E_ARG;
    RCCHK(set_begin(b));
    mp3d_batch::LoudnessSink &k = b->ld;
    if (!on) {
        k.off();
        return MP3D_OK;
    }
    std::unique_ptr<LdTab> tab(new LdTab);
    ld_build(b->rs.f.hz, b->rs.ch, *tab);
    const size_t ns = (size_t)b->max_streams;
    int r = k.tab.grow(b, sizeof(LdTab));
    if (!r) r = k.st.grow(b, sizeof(LdState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(LdPlan) * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.pk.grow(b, sizeof(float) * ns);
    if (!r) r = k.lu.grow(b, sizeof(float) * ns);
    if (!r) r = k.endst.grow(b, sizeof(double) * 8 * ns);
    if (!r) r = hip_rc(hipMemcpyAsync(k.tab, tab.get(), sizeof(LdTab), hipMemcpyHostToDevice, b->own));
    /* setting the sink restarts every stream's loudness state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(LdState) * ns, b->own));
    r = set_end(b, k, r); /* (tab is read until here) */
    k.on = !r;
    k.H = r ? 0 : tab->H;
    return r;
}

/* the most complete blocks S new samples can close on top of an open block */
static long long ld_bound(long long S, int H) { return (H - 1 + S) / H; }

/* The loudness stage on stream s: dsmp [n][sstride][channels] samples and
 * dcin [n] counts are device memory; blocks, block_count and peak are the
 * caller's (host or device; peak may be NULL).  Returns after the work is
 * queued when all of them are device memory, else when it is done. */
static int ld_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n, float *blocks,
                  long long block_stride, int *block_count, float *peak, int flags, hipStream_t s) {
    mp3d_batch::LoudnessSink &k = b->ld;
    const bool out_dev = is_device_ptr(blocks, b->device);
    const long long stride = std::min(block_stride, ld_bound(sstride, k.H));
    const long long tiles = std::max<long long>(1, (sstride + MP3D_LD_TILE - 1) / MP3D_LD_TILE);
    if (tiles * n > 0x7fffffffLL) return MP3D_E_CAPACITY;
    if (out_dev && (uintptr_t)blocks % sizeof(float)) return MP3D_E_ARG;
    CallerOut<int32_t> cnt;
    CallerOut<float> pk;
    RCCHK(cnt.pick(b, (int32_t *)block_count, k.cnt));
    RCCHK(pk.pick(b, peak, k.pk));
    const size_t nt = (size_t)n * (size_t)tiles;
    int r = MP3D_OK;
    if (!out_dev) r = k.out.grow(b, sizeof(float) * (size_t)stride * n + 16);
    if (!r) r = k.tz.grow(b, sizeof(double) * 8 * nt);
    if (!r) r = k.entry.grow(b, sizeof(double) * 8 * nt);
    if (!r) r = k.part.grow(b, sizeof(double) * MP3D_LD_TILE_BLOCKS * nt);
    if (!r) r = k.tpeak.grow(b, sizeof(float) * nt);
    if (r) return r;
    float *dout = out_dev ? blocks : (float *)k.out.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_loudness(dsmp, dcin, k.st, k.plan, k.tab, k.H, b->rs.ch, k.tz, k.entry, k.part, k.tpeak, k.endst, dout,
                        cnt.dev, pk.dev ? pk.dev : k.pk.p, n, sstride, out_dev ? block_stride : stride, (int)tiles,
                        (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    if (pk.host) {
        HIPCHK(pk.copy_back(n, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return deliver_rows(s, n, sizeof(float), dout, stride, blocks, block_stride, cnt.dev, block_count, out_dev,
                        !cnt.host);
}

extern "C" int mp3d_batch_decode_loudness(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                          const uint32_t *sizes, int n, int F, float *blocks, long long block_stride,
                                          int *block_count, float *peak, int flags, mp3d_frame_info *infos,
                                          void *hip_stream) {
    if (!b || !b->ld.on || !blocks || !block_count || block_stride < 0) return MP3D_E_ARG;
    long long S;
    hipStream_t s;
    RCCHK(decode_to_stage(b, b->ld, frames, offsets, sizes, n, F, flags, infos, hip_stream, &S, &s));
    CallEnd done{b, s};
    return ld_run(b, b->ld.smp, b->ld.cin, S, n, blocks, block_stride, block_count, peak, flags, s);
}

extern "C" int mp3d_batch_loudness(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts, int n,
                                   float *blocks, long long block_stride, int *block_count, float *peak, int flags,
                                   void *hip_stream) {
    if (!b || !b->ld.on || !counts || !blocks || !block_count || sample_stride < 0 || block_stride < 0 ||
        (flags & ~MP3D_PACK_FLUSH))
        return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > 0x7fffffffLL) return MP3D_E_ARG; /* counts are int */
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp;
    const int32_t *dcin;
    bool host_in = false;
    const size_t frame = sizeof(float) * b->rs.ch;
    RCCHK(stage_inputs(b, b->ld, samples, sample_stride, frame, counts, n, s, &dsmp, &dcin, &host_in));
    RCCHK(ld_run(b, dsmp, dcin, sample_stride, n, blocks, block_stride, block_count, peak, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_loudness_integrated(mp3d_batch *b, const float *blocks, long long block_stride,
                                              const int *counts, int n, float *lufs, void *hip_stream) {
    if (!b || !b->ld.on || !counts || !lufs || block_stride < 0 || (!blocks && block_stride) || n <= 0)
        return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    mp3d_batch::LoudnessSink &k = b->ld;
    /* a host caller's rows are staged in out, their counts in cnt */
    const float *dz = blocks;
    const int32_t *dc;
    bool host = false;
    if (block_stride && !is_device_ptr(blocks, b->device)) {
        RCCHK(k.out.grow(b, sizeof(float) * (size_t)block_stride * n + 16));
        HIPCHK(hipMemcpyAsync(k.out, blocks, sizeof(float) * (size_t)block_stride * n, hipMemcpyDefault, s));
        dz = (const float *)k.out.p;
        host = true;
    } else if (block_stride && (uintptr_t)blocks % sizeof(float)) {
        return MP3D_E_ARG;
    }
    RCCHK(caller_in(b, (const int32_t *)counts, n, k.cnt, s, &dc, &host));
    CallerOut<float> lu;
    RCCHK(lu.pick(b, lufs, k.lu));
    RCCHK(stage_launch(b, nullptr, s, [&] { launch_loudness_gate(dz, block_stride, dc, lu.dev, n, s); }));
    HIPCHK(lu.copy_back(n, s));
    if (host || lu.host) HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

extern "C" int mp3d_batch_loudness_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->ld.tm, us) : MP3D_E_ARG;
}
