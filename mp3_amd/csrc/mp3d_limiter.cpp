/*
 * mp3d_limiter.cpp -- the look-ahead true-peak limiter on top of the packed
 * sink: its constants and the calls around mp3d_limiter.hip (include/mp3d.h
 * "limiter").
 */
#include "mp3d_host.h"

using namespace mp3d;

static int lim_ahead(int hz) { return (hz + 50) / 100; }

/* the largest stride of either side: counts are int, and so are a call's
 * emitted indices (its samples + A + 6) rounded up to whole tiles, and the
 * frame indices of a tile's span (up to n_in + A + 6), all in frames; element
 * offsets are 64 bits in the kernels */
static const long long LIM_MAX_STRIDE = 0x7fffffffLL - 2 * MP3D_LIM_TILE;
static_assert(MP3D_LIM_AHEAD(MP3D_LIM_AMAX) + MP3D_LIM_TILE <= 2 * MP3D_LIM_TILE, "the margin holds A + 6 and a tile's rounding");

extern "C" long long mp3d_limiter_lookahead(int hz) {
    if (rs_rate_index(hz) < 0) return MP3D_E_ARG;
    return lim_ahead(hz);
}

extern "C" long long mp3d_limiter_max_samples(int hz, long long in_samples) {
    if (rs_rate_index(hz) < 0 || in_samples < 0 || in_samples > 0x7fffffffLL) return MP3D_E_ARG;
    return in_samples + MP3D_LIM_AHEAD(lim_ahead(hz));
}

extern "C" int mp3d_batch_set_limiter(mp3d_batch *b, int on, double ceiling_db) {
    if (!b || (on && (!b->rs.f.hz || !(ceiling_db >= -20.0 && ceiling_db <= 0.0)))) return MP3D_E_ARG;
    RCCHK(set_begin(b));
    mp3d_batch::LimiterSink &k = b->lm;
    if (!on) {
        k.off();
        return MP3D_OK;
    }
    static_assert(MP3D_LIM_AMAX == (48000 + 50) / 100, "the largest rate's look-ahead");
    float taps[MP3D_TP_R * MP3D_TP_TAPS];
    (void)mp3d_truepeak_filter(taps, MP3D_TP_R * MP3D_TP_TAPS);
    const size_t ns = (size_t)b->max_streams;
    int r = k.taps.grow(b, sizeof(taps));
    if (!r) r = k.st.grow(b, sizeof(LimState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(LimPlan) * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.gg.grow(b, sizeof(float) * ns);
    if (!r) r = k.grd.grow(b, sizeof(float) * ns);
    if (!r) r = hip_rc(hipMemcpyAsync(k.taps, taps, sizeof(taps), hipMemcpyHostToDevice, b->own));
    /* setting the limiter restarts every stream's limiter state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(LimState) * ns, b->own));
    r = set_end(b, k, r); /* (taps is read until here) */
    k.on = !r;
    k.A = r ? 0 : lim_ahead(b->rs.f.hz);
    k.c = r ? 1.0f : (float)pow(10.0, ceiling_db / 20.0);
    return r;
}

/* The limiter stage on stream s: dsmp [n][sstride][channels] samples, dcin [n]
 * counts and dgain [n] (or null) are device memory; out, out_count and gr
 * (or null) are the caller's (host or device).  Returns after the work is
 * queued when all of them are device memory, else when it is done. */
static int lim_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n, const float *dgain,
                   void *out, int f32, long long out_stride, int *out_count, float *gr, int flags, hipStream_t s) {
    mp3d_batch::LimiterSink &k = b->lm;
    const int oc = b->rs.ch;
    const size_t eb = f32 ? sizeof(float) : sizeof(int16_t);
    const bool out_dev = is_device_ptr(out, b->device);
    /* (the alignment rule of mp3d_batch_apply_gain's out) */
    if (out_dev && (uintptr_t)out % (eb * oc)) return MP3D_E_ARG;
    CallerOut<int32_t> cnt;
    CallerOut<float> gro;
    RCCHK(cnt.pick(b, (int32_t *)out_count, k.cnt));
    RCCHK(gro.pick(b, gr, k.grd));
    /* no call emits more than its samples plus the A + 6 it found pending */
    const long long most = sstride + MP3D_LIM_AHEAD(k.A), stride = std::min(out_stride, most);
    const long long tiles = std::max<long long>(1, (std::min(most, out_stride) + MP3D_LIM_TILE - 1) / MP3D_LIM_TILE);
    /* one block per (stream, tile): the grid's blocks fit int and its threads 32 bits */
    if (tiles * n > 0x7fffffffLL || tiles * n * MP3D_LIM_THREADS > 0xffffffffLL) return MP3D_E_CAPACITY;
    RCCHK(k.tile.grow(b, sizeof(float) * (size_t)n * (size_t)tiles));
    if (!out_dev) RCCHK(k.out.grow(b, eb * oc * (size_t)stride * n + 16));
    void *dout = out_dev ? out : k.out.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_limiter(dsmp, dcin, k.st, k.plan, k.taps, dgain, dout, cnt.dev, k.tile, gro.dev, f32 != 0, oc, n, sstride,
                       out_dev ? out_stride : stride, (int)tiles, k.A, k.c, (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    HIPCHK(gro.copy_back(n, s));
    RCCHK(deliver_rows(s, n, eb * oc, dout, stride, out, out_stride, cnt.dev, out_count, out_dev, !cnt.host));
    if (gro.host) HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

extern "C" int mp3d_batch_limit(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts, int n,
                                const float *gain, void *out, int f32, long long out_stride, int *out_count, float *gr,
                                int flags, void *hip_stream) {
    if (!b || !b->lm.on || !counts || !out || !out_count || sample_stride < 0 || out_stride < 0 ||
        (flags & ~MP3D_PACK_FLUSH))
        return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > LIM_MAX_STRIDE || out_stride > LIM_MAX_STRIDE) return MP3D_E_ARG;
    const size_t frame = sizeof(float) * b->rs.ch, row = frame * (size_t)sample_stride;
    const size_t orow = (f32 ? sizeof(float) : sizeof(int16_t)) * (size_t)out_stride * b->rs.ch;
    /* a tile reads its halo after its neighbours wrote their outputs: not in place */
    const uintptr_t s0 = (uintptr_t)samples, o0 = (uintptr_t)out;
    if (row && orow && s0 < o0 + orow * n && o0 < s0 + row * n) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp, *dg;
    const int32_t *dcin;
    bool host_in = false;
    RCCHK(stage_inputs(b, b->lm, samples, sample_stride, frame, counts, n, s, &dsmp, &dcin, &host_in));
    RCCHK(caller_in(b, gain, n, b->lm.gg, s, &dg, &host_in));
    RCCHK(lim_run(b, dsmp, dcin, sample_stride, n, dg, out, f32, out_stride, out_count, gr, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_decode_limited(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                         const uint32_t *sizes, int n, int F, const float *gain, void *out, int f32,
                                         long long out_stride, int *out_count, float *gr, int flags,
                                         mp3d_frame_info *infos, void *hip_stream) {
    if (!b || !b->lm.on || !out || !out_count || out_stride < 0 || out_stride > LIM_MAX_STRIDE) return MP3D_E_ARG;
    long long S;
    hipStream_t s;
    RCCHK(decode_to_stage(b, b->lm, frames, offsets, sizes, n, F, flags, infos, hip_stream, &S, &s));
    CallEnd done{b, s};
    const float *dg;
    bool host_in = false;
    RCCHK(caller_in(b, gain, n, b->lm.gg, s, &dg, &host_in));
    RCCHK(lim_run(b, b->lm.smp, b->lm.cin, S, n, dg, out, f32, out_stride, out_count, gr, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's gains are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_limiter_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->lm.tm, us) : MP3D_E_ARG;
}
