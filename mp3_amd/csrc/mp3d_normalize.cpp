/*
 * mp3d_normalize.cpp -- true peak and gain on top of the packed sink: the
 * oversampling filter's design, and the calls around mp3d_normalize.hip
 * (include/mp3d.h "true peak and gain").
 */
#include "mp3d_host.h"

using namespace mp3d;

/* modified Bessel function of the first kind, order 0: its power series */
static double tp_i0(double x) {
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

/* the filter of include/mp3d.h: taps[4][12] */
static void tp_design(float *taps) {
    const double beta = 6.0, half = MP3D_TP_TAPS / 2.0;
    for (int j = 0; j < MP3D_TP_TAPS; j++) taps[j] = j == MP3D_TP_PRE ? 1.0f : 0.0f;
    for (int p = 1; p < MP3D_TP_R; p++) {
        double h[MP3D_TP_TAPS], sum = 0.0;
        for (int j = 0; j < MP3D_TP_TAPS; j++) {
            const double t = (double)p / MP3D_TP_R - (double)(j - MP3D_TP_PRE), u = t / half;
            const double w = fabs(t) < half ? tp_i0(beta * sqrt(1.0 - u * u)) / tp_i0(beta) : 0.0;
            h[j] = sin(M_PI * t) / (M_PI * t) * w; /* (t is never 0 for p > 0) */
            sum += h[j];
        }
        for (int j = 0; j < MP3D_TP_TAPS; j++) taps[p * MP3D_TP_TAPS + j] = (float)(h[j] / sum);
    }
}

extern "C" long long mp3d_truepeak_filter(float *taps, size_t cap) {
    const long long n = MP3D_TP_R * MP3D_TP_TAPS;
    if (taps) {
        if ((long long)cap < n) return MP3D_E_ARG;
        tp_design(taps);
    }
    return n;
}

extern "C" int mp3d_batch_set_true_peak(mp3d_batch *b, int on) {
    if (!b || (on && !b->rs.f.hz)) return MP3D_E_ARG;
    RCCHK(set_begin(b));
    mp3d_batch::TruePeakTap &k = b->nm;
    if (!on) {
        k.off();
        return MP3D_OK;
    }
    float taps[MP3D_TP_R * MP3D_TP_TAPS];
    tp_design(taps);
    const size_t ns = (size_t)b->max_streams;
    int r = k.taps.grow(b, sizeof(taps));
    if (!r) r = k.st.grow(b, sizeof(TpState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(TpPlan) * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.tp.grow(b, sizeof(float) * ns);
    if (!r) r = hip_rc(hipMemcpyAsync(k.taps, taps, sizeof(taps), hipMemcpyHostToDevice, b->own));
    /* setting the tap restarts every stream's true-peak state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(TpState) * ns, b->own));
    r = set_end(b, k, r); /* (taps is read until here) */
    k.on = !r;
    return r;
}

/* The true-peak stage on stream s: dsmp [n][sstride][channels] samples and
 * dcin [n] counts are device memory; tpeak is the caller's (host or device).
 * Returns after the work is queued when it is device memory, else when it is
 * done. */
static int tp_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n, float *tpeak,
                  int flags, hipStream_t s) {
    mp3d_batch::TruePeakTap &k = b->nm;
    /* a call emits at most its samples plus the POST a flush releases */
    const long long tiles = std::max<long long>(1, (sstride + MP3D_TP_POST + MP3D_TP_TILE - 1) / MP3D_TP_TILE);
    if (tiles * n > 0x7fffffffLL) return MP3D_E_CAPACITY;
    CallerOut<float> tp;
    RCCHK(tp.pick(b, tpeak, k.tp));
    RCCHK(k.tile.grow(b, sizeof(float) * (size_t)n * (size_t)tiles));
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_true_peak(dsmp, dcin, k.st, k.plan, k.taps, k.tile, tp.dev, n, sstride, b->rs.ch, (int)tiles,
                         (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    if (tp.host) {
        HIPCHK(tp.copy_back(n, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return MP3D_OK;
}

/* the largest sample_stride of the tap and of mp3d_batch_apply_gain: counts
 * are int, and a call's emitted indices (its samples + POST) are too */
static const long long TP_MAX_STRIDE = 0x7fffffffLL - MP3D_TP_TILE;

extern "C" int mp3d_batch_true_peak(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                    int n, float *tpeak, int flags, void *hip_stream) {
    if (!b || !b->nm.on || !counts || !tpeak || sample_stride < 0 || (flags & ~MP3D_PACK_FLUSH)) return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > TP_MAX_STRIDE) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp;
    const int32_t *dcin;
    bool host_in = false;
    const size_t frame = sizeof(float) * b->rs.ch;
    RCCHK(stage_inputs(b, b->nm, samples, sample_stride, frame, counts, n, s, &dsmp, &dcin, &host_in));
    RCCHK(tp_run(b, dsmp, dcin, sample_stride, n, tpeak, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_decode_measure(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                         const uint32_t *sizes, int n, int F, float *blocks, long long block_stride,
                                         int *block_count, float *peak, float *tpeak, int flags, mp3d_frame_info *infos,
                                         void *hip_stream) {
    if (!b || !b->ld.on || !b->nm.on || !tpeak) return MP3D_E_ARG;
    /* the loudness call decodes into the handle's samples and counts and
     * leaves them there: the tap runs on the same ones, after it */
    RCCHK(mp3d_batch_decode_loudness(b, frames, offsets, sizes, n, F, blocks, block_stride, block_count, peak, flags,
                                     infos, hip_stream));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    return tp_run(b, b->ld.smp, b->ld.cin, stage_stride(b, F), n, tpeak, flags, s);
}

extern "C" int mp3d_batch_true_peak_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->nm.tm, us) : MP3D_E_ARG;
}

extern "C" int mp3d_batch_normalize_gain(mp3d_batch *b, const float *lufs, const float *tpeak, int n,
                                         double target_lufs, double max_dbtp, float *gain, void *hip_stream) {
    if (!b || !lufs || !gain || n <= 0 || !std::isfinite(target_lufs) || !std::isfinite(max_dbtp)) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    mp3d_batch::GainCalls &k = b->ga;
    const float *dl, *dt;
    bool host = false;
    RCCHK(caller_in(b, lufs, n, k.lu, s, &dl, &host));
    RCCHK(caller_in(b, tpeak, n, k.gtp, s, &dt, &host));
    CallerOut<float> gn;
    RCCHK(gn.pick(b, gain, k.gain));
    RCCHK(stage_launch(b, nullptr, s, [&] {
        launch_gain_calc(dl, dt, gn.dev, n, target_lufs, pow(10.0, max_dbtp / 20.0), s);
    }));
    HIPCHK(gn.copy_back(n, s));
    if (host || gn.host) HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

extern "C" int mp3d_batch_apply_gain(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                     int n, const float *gain, void *out, int f32, void *hip_stream) {
    if (!b || !b->rs.f.hz || !counts || !gain || !out || sample_stride < 0) return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (!f32 && out == (const void *)samples) return MP3D_E_ARG; /* in place is for float32 */
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > TP_MAX_STRIDE) return MP3D_E_ARG;
    const int oc = b->rs.ch;
    const size_t eb = f32 ? sizeof(float) : sizeof(int16_t);
    const long long chunks = std::max<long long>(1, (sample_stride * oc + MP3D_GA_CHUNK - 1) / MP3D_GA_CHUNK);
    if (chunks * n > 0x7fffffffLL) return MP3D_E_CAPACITY;
    const bool out_dev = is_device_ptr(out, b->device);
    /* (the alignment rule of mp3d_batch_decode_packed's out) */
    if (out_dev && (uintptr_t)out % (eb * oc)) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    mp3d_batch::GainCalls &k = b->ga;
    const float *dsmp, *dg;
    const int32_t *dcin;
    bool host_in = false;
    RCCHK(stage_inputs(b, k, samples, sample_stride, sizeof(float) * oc, counts, n, s, &dsmp, &dcin, &host_in));
    RCCHK(caller_in(b, gain, n, k.gg, s, &dg, &host_in));
    /* cnt: each stream's count clamped to the stride */
    RCCHK(k.cnt.grow(b, sizeof(int32_t) * (size_t)b->max_streams));
    if (!out_dev) RCCHK(k.out.grow(b, eb * oc * (size_t)sample_stride * n + 16));
    void *dout = out_dev ? out : k.out.p;
    RCCHK(stage_launch(b, nullptr, s, [&] {
        launch_gain_apply(dsmp, dcin, dg, dout, k.cnt, f32 != 0, oc, n, sample_stride, (int)chunks, s);
    }));
    /* a host out: each stream's own rows, by its clamped count */
    RCCHK(deliver_rows(s, n, eb * oc, dout, sample_stride, out, sample_stride, k.cnt, nullptr, out_dev, true));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

