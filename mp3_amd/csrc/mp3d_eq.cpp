/*
 * mp3d_eq.cpp -- the equaliser sink on top of the packed sink: the cookbook
 * design of its sections, the state-transition tables of the cascade, and the
 * calls around mp3d_eq.hip (include/mp3d.h "equaliser sink"; DESIGN.md
 * section 4j).
 */
#include "mp3d_host.h"

#include <memory>

using namespace mp3d;

static_assert(MP3D_EQ_BANDS == MP3D_EQ_MAX_BANDS, "mp3d_eq.h and include/mp3d.h agree");

static bool eq_in(double x, double lo, double hi) { return x >= lo && x <= hi; } /* (false for a NaN) */

/* the sections of include/mp3d.h for fs = hz: b0 b1 b2 a1 a2 per stage */
static int eq_design(int hz, const mp3d_eq_band *bands, int n, double preamp_db, double *coef) {
    if (rs_rate_index(hz) < 0 || !bands || n < 1 || n > MP3D_EQ_MAX_BANDS || !eq_in(preamp_db, -24.0, 24.0))
        return MP3D_E_ARG;
    for (int k = 0; k < n; k++) {
        const mp3d_eq_band &d = bands[k];
        if (d.type < MP3D_EQ_PEAK || d.type > MP3D_EQ_LOW_PASS || !eq_in(d.f0_hz, 20.0, 0.45 * hz) ||
            !eq_in(d.q, 0.1, 16.0) || !eq_in(d.gain_db, -24.0, 24.0))
            return MP3D_E_ARG;
    }
    for (int k = 0; k < n; k++) {
        const mp3d_eq_band &d = bands[k];
        const long double w0 = 2.0L * M_PIl * (long double)d.f0_hz / (long double)hz;
        const long double cs = cosl(w0), alpha = sinl(w0) / (2.0L * (long double)d.q);
        const long double A = powl(10.0L, (long double)d.gain_db / 40.0L), sq = 2.0L * sqrtl(A) * alpha;
        long double b[3], a[3];
        switch (d.type) {
        case MP3D_EQ_PEAK:
            b[0] = 1.0L + alpha * A, b[1] = -2.0L * cs, b[2] = 1.0L - alpha * A;
            a[0] = 1.0L + alpha / A, a[1] = -2.0L * cs, a[2] = 1.0L - alpha / A;
            break;
        case MP3D_EQ_LOW_SHELF:
            b[0] = A * ((A + 1.0L) - (A - 1.0L) * cs + sq);
            b[1] = 2.0L * A * ((A - 1.0L) - (A + 1.0L) * cs);
            b[2] = A * ((A + 1.0L) - (A - 1.0L) * cs - sq);
            a[0] = (A + 1.0L) + (A - 1.0L) * cs + sq;
            a[1] = -2.0L * ((A - 1.0L) + (A + 1.0L) * cs);
            a[2] = (A + 1.0L) + (A - 1.0L) * cs - sq;
            break;
        case MP3D_EQ_HIGH_SHELF:
            b[0] = A * ((A + 1.0L) + (A - 1.0L) * cs + sq);
            b[1] = -2.0L * A * ((A - 1.0L) + (A + 1.0L) * cs);
            b[2] = A * ((A + 1.0L) + (A - 1.0L) * cs - sq);
            a[0] = (A + 1.0L) - (A - 1.0L) * cs + sq;
            a[1] = 2.0L * ((A - 1.0L) - (A + 1.0L) * cs);
            a[2] = (A + 1.0L) - (A - 1.0L) * cs - sq;
            break;
        case MP3D_EQ_HIGH_PASS:
            b[0] = (1.0L + cs) / 2.0L, b[1] = -(1.0L + cs), b[2] = (1.0L + cs) / 2.0L;
            a[0] = 1.0L + alpha, a[1] = -2.0L * cs, a[2] = 1.0L - alpha;
            break;
        default: /* MP3D_EQ_LOW_PASS */
            b[0] = (1.0L - cs) / 2.0L, b[1] = 1.0L - cs, b[2] = (1.0L - cs) / 2.0L;
            a[0] = 1.0L + alpha, a[1] = -2.0L * cs, a[2] = 1.0L - alpha;
            break;
        }
        const long double g = k ? 1.0L : powl(10.0L, (long double)preamp_db / 20.0L);
        double *c = coef + 5 * k;
        for (int i = 0; i < 3; i++) c[i] = (double)(b[i] * g / a[0]);
        c[3] = (double)(a[1] / a[0]);
        c[4] = (double)(a[2] / a[0]);
    }
    return MP3D_OK;
}

extern "C" long long mp3d_eq_design(int hz, const mp3d_eq_band *bands, int n_bands, double preamp_db, double *coef,
                                    size_t cap) {
    double c[5 * MP3D_EQ_MAX_BANDS];
    RCCHK(eq_design(hz, bands, n_bands, preamp_db, c));
    if (coef) {
        if (cap < (size_t)(5 * n_bands)) return MP3D_E_ARG;
        memcpy(coef, c, sizeof(double) * 5 * (size_t)n_bands);
    }
    return 5 * n_bands;
}

/* r = a b for n x n row-major matrices (r may be a or b) */
static void eq_mul(const std::vector<long double> &a, const std::vector<long double> &b, std::vector<long double> &r,
                   int n) {
    std::vector<long double> o((size_t)n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            long double acc = 0;
            for (int k = 0; k < n; k++) acc += a[(size_t)i * n + k] * b[(size_t)k * n + j];
            o[(size_t)i * n + j] = acc;
        }
    r.swap(o);
}

/* The state transitions for a zero input (the kernels' eq_step with v = 0)
 * and their powers, in long double: each stage's 2 x 2 A_k^(SEG t) into
 * t.apow, the cascade's 2K x 2K A^(TILE t) into tpow, t = 0 .. 64. */
static void eq_build(const double *coef, int K, int ch, EqTab &t, std::vector<double> &tpow) {
    memset(&t, 0, sizeof(t));
    t.K = K, t.ch = ch;
    memcpy(t.coef, coef, sizeof(double) * 5 * (size_t)K);
    static_assert(MP3D_EQ_SEG == 16 && MP3D_EQ_TILE == 4096, "A^SEG by four squarings, A^TILE by twelve");
    for (int k = 0; k < K; k++) {
        const double *c = coef + 5 * k;
        std::vector<long double> seg = {-(long double)c[3], 1.0L, -(long double)c[4], 0.0L}, p = {1.0L, 0.0L, 0.0L, 1.0L};
        for (int i = 0; i < 4; i++) eq_mul(seg, seg, seg, 2);
        for (int d = 0; d <= 64; d++) {
            for (int i = 0; i < 4; i++) t.apow[k][d][i] = (double)p[i];
            eq_mul(p, seg, p, 2);
        }
    }
    const int n = 2 * K;
    std::vector<long double> A((size_t)n * n), q((size_t)n * n, 0.0L);
    for (int j = 0; j < n; j++) {
        long double u = 0.0L; /* the stage's input: the stage before's output */
        for (int k = 0; k < K; k++) {
            const double *c = coef + 5 * k;
            const long double s1 = 2 * k == j ? 1.0L : 0.0L, s2 = 2 * k + 1 == j ? 1.0L : 0.0L;
            const long double o = (long double)c[0] * u + s1;
            A[(size_t)(2 * k) * n + j] = (long double)c[1] * u - (long double)c[3] * o + s2;
            A[(size_t)(2 * k + 1) * n + j] = (long double)c[2] * u - (long double)c[4] * o;
            u = o;
        }
    }
    for (int i = 0; i < 12; i++) eq_mul(A, A, A, n);
    for (int i = 0; i < n; i++) q[(size_t)i * n + i] = 1.0L;
    tpow.resize((size_t)65 * n * n);
    for (int d = 0; d <= 64; d++) {
        for (int i = 0; i < n * n; i++) tpow[(size_t)d * n * n + i] = (double)q[i];
        eq_mul(q, A, q, n);
    }
}

extern "C" int mp3d_batch_set_eq(mp3d_batch *b, const mp3d_eq_band *bands, int n_bands, double preamp_db) {
    if (!b || n_bands < 0) return MP3D_E_ARG;
    mp3d_batch::EqSink &k = b->eq;
    if (!n_bands) {
        RCCHK(set_begin(b));
        k.off();
        return MP3D_OK;
    }
    if (!b->rs.f.hz) return MP3D_E_ARG;
    double coef[5 * MP3D_EQ_MAX_BANDS];
    RCCHK(eq_design(b->rs.f.hz, bands, n_bands, preamp_db, coef)); /* before anything changes */
    std::unique_ptr<EqTab> tab(new EqTab);
    std::vector<double> tpow;
    eq_build(coef, n_bands, b->rs.ch, *tab, tpow);
    RCCHK(set_begin(b));
    const size_t ns = (size_t)b->max_streams, tb = sizeof(double) * tpow.size();
    int r = k.tab.grow(b, sizeof(EqTab));
    if (!r) r = k.tpow.grow(b, tb);
    if (!r) r = k.st.grow(b, sizeof(EqState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(EqPlan) * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    if (!r) r = hip_rc(hipMemcpyAsync(k.tab, tab.get(), sizeof(EqTab), hipMemcpyHostToDevice, b->own));
    if (!r) r = hip_rc(hipMemcpyAsync(k.tpow, tpow.data(), tb, hipMemcpyHostToDevice, b->own));
    /* setting the curve restarts every stream's equaliser state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(EqState) * ns, b->own));
    r = set_end(b, k, r); /* (tab and tpow are read until here) */
    k.K = r ? 0 : n_bands;
    return r;
}

/* The equaliser stage on stream s: dsmp [n][sstride][channels] samples and
 * dcin [n] counts are device memory; out and out_count are the caller's (host
 * or device).  Returns after the work is queued when both are device memory,
 * else when it is done. */
static int eq_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n, float *out,
                  long long out_stride, int *out_count, int flags, hipStream_t s) {
    mp3d_batch::EqSink &k = b->eq;
    const int oc = b->rs.ch;
    const bool out_dev = is_device_ptr(out, b->device);
    /* (the alignment rule of mp3d_batch_apply_gain's out) */
    if (out_dev && (uintptr_t)out % (sizeof(float) * oc)) return MP3D_E_ARG;
    CallerOut<int32_t> cnt;
    RCCHK(cnt.pick(b, (int32_t *)out_count, k.cnt));
    /* no call emits more than its samples */
    const long long stride = std::min(out_stride, sstride);
    const long long tiles = std::max<long long>(1, (stride + MP3D_EQ_TILE - 1) / MP3D_EQ_TILE);
    /* one block per (stream, tile): the grid's blocks fit int and its threads 32 bits */
    if (tiles * n > 0x7fffffffLL || tiles * n * MP3D_EQ_THREADS > 0xffffffffLL) return MP3D_E_CAPACITY;
    const size_t nt = sizeof(double) * MP3D_EQ_TSTRIDE * (size_t)n * (size_t)tiles;
    RCCHK(k.tz.grow(b, nt));
    RCCHK(k.entry.grow(b, nt));
    if (!out_dev) RCCHK(k.out.grow(b, sizeof(float) * oc * (size_t)stride * n + 16));
    float *dout = out_dev ? out : (float *)k.out.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_eq(dsmp, dcin, k.st, k.plan, k.tab, k.tpow, k.tz, k.entry, dout, cnt.dev, k.K, oc, n, sstride,
                  out_dev ? out_stride : stride, (int)tiles, (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    return deliver_rows(s, n, sizeof(float) * oc, dout, stride, out, out_stride, cnt.dev, out_count, out_dev,
                        !cnt.host);
}

extern "C" int mp3d_batch_eq(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts, int n,
                             float *out, long long out_stride, int *out_count, int flags, void *hip_stream) {
    if (!b || !b->eq.K || !counts || !out || !out_count || sample_stride < 0 || out_stride < 0 ||
        (flags & ~MP3D_PACK_FLUSH))
        return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > 0x7fffffffLL || out_stride > 0x7fffffffLL) return MP3D_E_ARG; /* counts are int */
    const size_t frame = sizeof(float) * b->rs.ch, row = frame * (size_t)sample_stride, orow = frame * (size_t)out_stride;
    /* a tile's block writes its results while other blocks still read their samples: not in place */
    const uintptr_t s0 = (uintptr_t)samples, o0 = (uintptr_t)out;
    if (row && orow && s0 < o0 + orow * n && o0 < s0 + row * n) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    /* the tiles are loaded a sample frame's multiple at a time */
    if (sample_stride && is_device_ptr(samples, b->device) && s0 % frame) return MP3D_E_ARG;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp;
    const int32_t *dcin;
    bool host_in = false;
    RCCHK(stage_inputs(b, b->eq, samples, sample_stride, frame, counts, n, s, &dsmp, &dcin, &host_in));
    RCCHK(eq_run(b, dsmp, dcin, sample_stride, n, out, out_stride, out_count, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_decode_equalized(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                           const uint32_t *sizes, int n, int F, float *out, long long out_stride,
                                           int *out_count, int flags, mp3d_frame_info *infos, void *hip_stream) {
    if (!b || !b->eq.K || !out || !out_count || out_stride < 0 || out_stride > 0x7fffffffLL) return MP3D_E_ARG;
    long long S;
    hipStream_t s;
    RCCHK(decode_to_stage(b, b->eq, frames, offsets, sizes, n, F, flags, infos, hip_stream, &S, &s));
    CallEnd done{b, s};
    return eq_run(b, b->eq.smp, b->eq.cin, S, n, out, out_stride, out_count, flags, s);
}

extern "C" int mp3d_batch_eq_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->eq.tm, us) : MP3D_E_ARG;
}
