/*
 * mp3d_pitch.cpp -- the pitch sink on top of the packed sink: its lag range
 * and bound, and the calls around mp3d_pitch.hip (include/mp3d.h "pitch
 * sink").
 */
#include "mp3d_host.h"

using namespace mp3d;

static int pt_hop(int hz) { return (hz + 50) / 100; }
static_assert(MP3D_PT_HMAX == (48000 + 50) / 100, "the largest rate's hop");
static_assert(MP3D_PT_TMAX == 48000 / 50 + 1, "the longest lag range");
static_assert(sizeof(mp3d_pitch_frame) == 16, "a record is four words");

static bool pt_fmin_ok(int hz, int fmin) { return fmin >= 50 && fmin + 1 <= 2000 && 4LL * (fmin + 1) <= hz; }
static bool pt_range_ok(int hz, int fmin, int fmax) {
    return fmin >= 50 && fmin < fmax && fmax <= 2000 && 4LL * fmax <= hz;
}
static int pt_T(int hz, int fmin) { return hz / fmin + 1; }
static int pt_span(int hz, int fmin) { return 2 * pt_hop(hz) + pt_T(hz, fmin); }

/* the bound of include/mp3d.h */
static long long pt_bound(int H, int SPAN, long long S) { return (S + SPAN + H - 2) / H; }

/* counts are int; a call's frames, rounded up to whole tiles, too */
static const long long PT_MAX_STRIDE = 0x7fffffffLL - 2 * MP3D_PT_HMAX;

extern "C" long long mp3d_pitch_span(int hz, int fmin_hz, int fmax_hz, int *tau_min, int *tau_max) {
    if (rs_rate_index(hz) < 0 || !pt_range_ok(hz, fmin_hz, fmax_hz)) return MP3D_E_ARG;
    if (tau_min) *tau_min = (hz + fmax_hz - 1) / fmax_hz;
    if (tau_max) *tau_max = hz / fmin_hz;
    return pt_span(hz, fmin_hz);
}

extern "C" long long mp3d_pitch_max_frames(int hz, long long in_samples, int fmin_hz) {
    if (rs_rate_index(hz) < 0 || in_samples < 0 || in_samples > 0x7fffffffLL || !pt_fmin_ok(hz, fmin_hz))
        return MP3D_E_ARG;
    return pt_bound(pt_hop(hz), pt_span(hz, fmin_hz), in_samples);
}

extern "C" int mp3d_batch_set_pitch(mp3d_batch *b, int on, int fmin_hz, int fmax_hz, int theta) {
    if (!b) return MP3D_E_ARG;
    if (on && (!b->rs.f.hz || !pt_range_ok(b->rs.f.hz, fmin_hz, fmax_hz) || theta < 1 || theta > 1024))
        return MP3D_E_ARG;
    RCCHK(set_begin(b));
    mp3d_batch::PitchSink &k = b->pt;
    if (!on) {
        k.off();
        return MP3D_OK;
    }
    const int hz = b->rs.f.hz;
    const size_t ns = (size_t)b->max_streams;
    int r = k.st.grow(b, sizeof(PtState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(PtPlan) * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    /* setting the sink restarts every stream's pitch state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(PtState) * ns, b->own));
    r = set_end(b, k, r);
    k.on = !r;
    k.H = r ? 0 : pt_hop(hz);
    k.T = r ? 0 : pt_T(hz, fmin_hz);
    k.tmin = r ? 0 : (hz + fmax_hz - 1) / fmax_hz;
    k.theta = r ? 0 : theta;
    return r;
}

/* The pitch stage on stream s: dsmp [n][sstride][channels] samples and dcin
 * [n] counts are device memory; pitch and pitch_count are the caller's (host
 * or device).  Returns after the work is queued when both are device memory,
 * else when it is done. */
static int pt_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n,
                  mp3d_pitch_frame *pitch, long long pitch_stride, int *pitch_count, int flags, hipStream_t s) {
    mp3d_batch::PitchSink &k = b->pt;
    const bool out_dev = is_device_ptr(pitch, b->device);
    if (out_dev && (uintptr_t)pitch % 8) return MP3D_E_ARG;
    CallerOut<int32_t> cnt;
    RCCHK(cnt.pick(b, (int32_t *)pitch_count, k.cnt));
    /* no call emits more than the bound; a block per tile of the frames it can emit */
    const long long bound = pt_bound(k.H, 2 * k.H + k.T, sstride), stride = std::min(pitch_stride, bound);
    const long long tiles = std::max<long long>(1, (bound + MP3D_PT_TILE - 1) / MP3D_PT_TILE);
    /* one block per (stream, tile): the grid's blocks fit int and its threads 32 bits */
    if (tiles * n > 0x7fffffffLL || tiles * n * MP3D_PT_THREADS > 0xffffffffLL) return MP3D_E_CAPACITY;
    if (!out_dev) RCCHK(k.out.grow(b, sizeof(mp3d_pitch_frame) * (size_t)stride * n + 16));
    mp3d_pitch_frame *dout = out_dev ? pitch : (mp3d_pitch_frame *)k.out.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_pitch(dsmp, dcin, k.st, k.plan, dout, cnt.dev, b->rs.ch, n, sstride, out_dev ? pitch_stride : stride,
                     (int)tiles, b->rs.f.hz, k.H, k.T, k.tmin, k.theta, (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    return deliver_rows(s, n, sizeof(mp3d_pitch_frame), dout, stride, pitch, pitch_stride, cnt.dev, pitch_count,
                        out_dev, !cnt.host);
}

extern "C" int mp3d_batch_pitch(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts, int n,
                                mp3d_pitch_frame *pitch, long long pitch_stride, int *pitch_count, int flags,
                                void *hip_stream) {
    if (!b || !b->pt.on || !counts || !pitch || !pitch_count || sample_stride < 0 || pitch_stride < 0 ||
        (flags & ~MP3D_PACK_FLUSH))
        return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > PT_MAX_STRIDE || pitch_stride > 0x7fffffffLL) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp;
    const int32_t *dcin;
    bool host_in = false;
    RCCHK(stage_inputs(b, b->pt, samples, sample_stride, sizeof(float) * b->rs.ch, counts, n, s, &dsmp, &dcin,
                       &host_in));
    RCCHK(pt_run(b, dsmp, dcin, sample_stride, n, pitch, pitch_stride, pitch_count, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_decode_pitch(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                       const uint32_t *sizes, int n, int F, mp3d_pitch_frame *pitch,
                                       long long pitch_stride, int *pitch_count, int flags, mp3d_frame_info *infos,
                                       void *hip_stream) {
    if (!b || !b->pt.on || !pitch || !pitch_count || pitch_stride < 0 || pitch_stride > 0x7fffffffLL)
        return MP3D_E_ARG;
    long long S;
    hipStream_t s;
    RCCHK(decode_to_stage(b, b->pt, frames, offsets, sizes, n, F, flags, infos, hip_stream, &S, &s));
    CallEnd done{b, s};
    return pt_run(b, b->pt.smp, b->pt.cin, S, n, pitch, pitch_stride, pitch_count, flags, s);
}

extern "C" int mp3d_batch_pitch_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->pt.tm, us) : MP3D_E_ARG;
}
