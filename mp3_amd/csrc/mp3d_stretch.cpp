/*
 * mp3d_stretch.cpp -- the tempo sink on top of the packed sink: the crossfade
 * table, the stride bound, and the calls around mp3d_stretch.hip
 * (include/mp3d.h "tempo sink").
 */
#include "mp3d_host.h"

using namespace mp3d;

static int st_hop(int hz) { return (hz + 50) / 100; }

static bool st_ratio_ok(int num, int den) {
    return num >= 1 && den >= 1 && num <= MP3D_ST_TEMPO_MAX && den <= MP3D_ST_TEMPO_MAX && num <= 2 * den &&
           den <= 2 * num;
}

static void st_window(int H, float *w) {
    for (int n = 0; n < H; n++) w[n] = (float)(0.5 - 0.5 * cos(M_PI * (n + 0.5) / H));
}

/* the bound of include/mp3d.h: ceil((S + 2H + D) den / num) */
static long long st_bound(int H, long long S, int num, int den) {
    return ((S + 2 * H + H / 2) * den + num - 1) / num;
}

extern "C" long long mp3d_stretch_window(int hz, float *w, size_t cap) {
    if (rs_rate_index(hz) < 0) return MP3D_E_ARG;
    const int H = st_hop(hz);
    if (w) {
        if (cap < (size_t)H) return MP3D_E_ARG;
        st_window(H, w);
    }
    return H;
}

extern "C" long long mp3d_stretch_max_samples(int out_hz, long long in_samples, int num, int den) {
    if (rs_rate_index(out_hz) < 0 || in_samples < 0 || in_samples > 0x7fffffffLL || !st_ratio_ok(num, den))
        return MP3D_E_ARG;
    return st_bound(st_hop(out_hz), in_samples, num, den);
}

extern "C" int mp3d_batch_set_stretch(mp3d_batch *b, int on) {
    if (!b || (on && !b->rs.f.hz)) return MP3D_E_ARG;
    RCCHK(set_begin(b));
    mp3d_batch::StretchSink &k = b->sx;
    if (!on) {
        k.off();
        return MP3D_OK;
    }
    const int H = st_hop(b->rs.f.hz);
    static_assert(MP3D_ST_HMAX == (48000 + 50) / 100, "the largest rate's hop");
    float w[MP3D_ST_HMAX];
    st_window(H, w);
    const size_t ns = (size_t)b->max_streams;
    std::vector<int32_t> one(2 * ns, 1); /* every slot at tempo 1/1 */
    int r = k.w.grow(b, sizeof(float) * MP3D_ST_HMAX);
    if (!r) r = k.st.grow(b, sizeof(StState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(StPlan) * ns);
    if (!r) r = k.tempo.grow(b, sizeof(int32_t) * 2 * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    if (!r) r = hip_rc(hipMemcpyAsync(k.w, w, sizeof(float) * H, hipMemcpyHostToDevice, b->own));
    if (!r) r = hip_rc(hipMemcpyAsync(k.tempo, one.data(), sizeof(int32_t) * 2 * ns, hipMemcpyHostToDevice, b->own));
    /* setting the sink restarts every stream's stretch state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(StState) * ns, b->own));
    r = set_end(b, k, r); /* (w and one are read until here) */
    k.on = !r;
    k.H = r ? 0 : H;
    return r;
}

extern "C" int mp3d_batch_set_tempo(mp3d_batch *b, int first, int n, const int *num, const int *den) {
    if (!b || !b->sx.on || first < 0 || n <= 0 || !num || !den) return MP3D_E_ARG;
    if ((long long)first + n > b->max_streams) return MP3D_E_CAPACITY;
    std::vector<int32_t> t(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        if (!st_ratio_ok(num[i], den[i])) return MP3D_E_ARG; /* before anything is written */
        t[2 * i] = num[i], t[2 * i + 1] = den[i];
    }
    return slots_set(b, [&](hipStream_t s) -> int {
        HIPCHK(hipMemcpyAsync(b->sx.tempo + 2 * (size_t)first, t.data(), sizeof(int32_t) * t.size(),
                              hipMemcpyHostToDevice, s));
        /* a new tempo is a new stream: the slots' stretch state restarts */
        HIPCHK(hipMemsetAsync(b->sx.st + first, 0, sizeof(StState) * (size_t)n, s));
        return MP3D_OK;
    });
}

/* The stretch stage on stream s: dsmp [n][sstride][channels] samples and dcin
 * [n] counts are device memory; out and out_count are the caller's (host or
 * device).  Returns after the work is queued when both are device memory,
 * else when it is done. */
static int st_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n, float *out,
                  long long out_stride, int *out_count, int flags, hipStream_t s) {
    mp3d_batch::StretchSink &k = b->sx;
    const int oc = b->rs.ch;
    const bool out_dev = is_device_ptr(out, b->device);
    /* (the alignment rule of mp3d_batch_apply_gain's out) */
    if (out_dev && (uintptr_t)out % (sizeof(float) * oc)) return MP3D_E_ARG;
    CallerOut<int32_t> cnt;
    RCCHK(cnt.pick(b, (int32_t *)out_count, k.cnt));
    /* no call emits more than the bound at the slowest tempo */
    const long long stride = std::min(out_stride, st_bound(k.H, sstride, 1, 2));
    if (!out_dev) RCCHK(k.out.grow(b, sizeof(float) * oc * (size_t)stride * n + 16));
    float *dout = out_dev ? out : (float *)k.out.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_stretch(dsmp, dcin, k.st, k.tempo, k.plan, k.w, dout, cnt.dev, n, sstride, out_dev ? out_stride : stride,
                       k.H, oc, (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    return deliver_rows(s, n, sizeof(float) * oc, dout, stride, out, out_stride, cnt.dev, out_count, out_dev, !cnt.host);
}

extern "C" int mp3d_batch_stretch(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts, int n,
                                  float *out, long long out_stride, int *out_count, int flags, void *hip_stream) {
    if (!b || !b->sx.on || !counts || !out || !out_count || sample_stride < 0 || out_stride < 0 ||
        (flags & ~MP3D_PACK_FLUSH))
        return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > 0x7fffffffLL || out_stride > 0x7fffffffLL) return MP3D_E_ARG; /* counts are int */
    const size_t frame = sizeof(float) * b->rs.ch, row = frame * (size_t)sample_stride, orow = frame * (size_t)out_stride;
    /* the stage reads a block's samples after it wrote earlier blocks: not in place */
    const uintptr_t s0 = (uintptr_t)samples, o0 = (uintptr_t)out;
    if (row && orow && s0 < o0 + orow * n && o0 < s0 + row * n) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp;
    const int32_t *dcin;
    bool host_in = false;
    RCCHK(stage_inputs(b, b->sx, samples, sample_stride, frame, counts, n, s, &dsmp, &dcin, &host_in));
    RCCHK(st_run(b, dsmp, dcin, sample_stride, n, out, out_stride, out_count, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_decode_stretched(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                           const uint32_t *sizes, int n, int F, float *out, long long out_stride,
                                           int *out_count, int flags, mp3d_frame_info *infos, void *hip_stream) {
    if (!b || !b->sx.on || !out || !out_count || out_stride < 0 || out_stride > 0x7fffffffLL) return MP3D_E_ARG;
    long long S;
    hipStream_t s;
    RCCHK(decode_to_stage(b, b->sx, frames, offsets, sizes, n, F, flags, infos, hip_stream, &S, &s));
    CallEnd done{b, s};
    return st_run(b, b->sx.smp, b->sx.cin, S, n, out, out_stride, out_count, flags, s);
}

extern "C" int mp3d_batch_stretch_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->sx.tm, us) : MP3D_E_ARG;
}
