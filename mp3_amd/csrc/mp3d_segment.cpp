/*
 * mp3d_segment.cpp -- the segment sink on top of the packed sink: its
 * threshold and bound, and the calls around mp3d_segment.hip (include/mp3d.h
 * "segment sink").
 */
#include "mp3d_host.h"

using namespace mp3d;

static int sg_hop(int hz) { return (hz + 50) / 100; }
static_assert(MP3D_SG_HMAX == (48000 + 50) / 100, "the largest rate's hop");

/* the largest hop energy: H samples at full scale */
static unsigned long long sg_full(int H) { return (unsigned long long)H << 30; }

static bool sg_hops_ok(int pause, int speech) {
    return pause >= 1 && pause <= MP3D_SG_MAXHOPS && speech >= 1 && speech <= MP3D_SG_MAXHOPS;
}

/* the most hops a call of S samples completes, the pending part hop included: ceil((S + H - 1) / H) */
static long long sg_hops(int H, long long S) { return (S + 2 * H - 2) / H; }

/* the bound of include/mp3d.h: 2 + K / (S + P) */
static long long sg_bound(int H, long long S, int pause, int speech) { return 2 + sg_hops(H, S) / (speech + pause); }

/* counts are int; a call's hops, rounded up to whole tiles, too */
static const long long SG_MAX_STRIDE = 0x7fffffffLL - 2 * MP3D_SG_HMAX;

static long long sg_threshold(int H, double db) {
    const double e = ceil((double)sg_full(H) * pow(10.0, db / 10.0));
    return e < 1.0 ? 1 : (long long)e;
}

extern "C" long long mp3d_segment_threshold(int hz, double db) {
    if (rs_rate_index(hz) < 0 || !(db >= -96.0 && db <= 0.0)) return MP3D_E_ARG;
    return sg_threshold(sg_hop(hz), db);
}

extern "C" long long mp3d_segment_max(int hz, long long in_samples, int pause_hops, int speech_hops) {
    if (rs_rate_index(hz) < 0 || in_samples < 0 || in_samples > 0x7fffffffLL || !sg_hops_ok(pause_hops, speech_hops))
        return MP3D_E_ARG;
    return sg_bound(sg_hop(hz), in_samples, pause_hops, speech_hops);
}

extern "C" int mp3d_batch_set_segments(mp3d_batch *b, int on, int pause_hops, int speech_hops, int pad_hops) {
    if (!b) return MP3D_E_ARG;
    if (on && (!b->rs.f.hz || !sg_hops_ok(pause_hops, speech_hops) || pad_hops < 0 || 2 * pad_hops > pause_hops))
        return MP3D_E_ARG;
    RCCHK(set_begin(b));
    mp3d_batch::SegmentSink &k = b->sg;
    if (!on) {
        k.off();
        return MP3D_OK;
    }
    const int H = sg_hop(b->rs.f.hz);
    const size_t ns = (size_t)b->max_streams;
    std::vector<uint64_t> thr(ns, (uint64_t)sg_threshold(H, -40.0)); /* every slot at -40 dBFS */
    int r = k.st.grow(b, sizeof(SgState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(SgPlan) * ns);
    if (!r) r = k.thr.grow(b, sizeof(uint64_t) * ns);
    if (!r) r = k.part.grow(b, sizeof(uint64_t) * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    if (!r) r = hip_rc(hipMemcpyAsync(k.thr, thr.data(), sizeof(uint64_t) * ns, hipMemcpyHostToDevice, b->own));
    /* setting the sink restarts every stream's segment state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(SgState) * ns, b->own));
    r = set_end(b, k, r); /* (thr is read until here) */
    k.on = !r;
    k.H = r ? 0 : H;
    k.P = r ? 0 : pause_hops, k.S = r ? 0 : speech_hops, k.pad = r ? 0 : pad_hops;
    return r;
}

extern "C" int mp3d_batch_set_segment_threshold(mp3d_batch *b, int first, int n, const unsigned long long *thr) {
    if (!b || !b->sg.on || first < 0 || n <= 0 || !thr) return MP3D_E_ARG;
    if ((long long)first + n > b->max_streams) return MP3D_E_CAPACITY;
    std::vector<uint64_t> t((size_t)n);
    for (int i = 0; i < n; i++) {
        if (thr[i] < 1 || thr[i] > sg_full(b->sg.H)) return MP3D_E_ARG; /* before anything is written */
        t[i] = thr[i];
    }
    return slots_set(b, [&](hipStream_t s) -> int {
        HIPCHK(hipMemcpyAsync(b->sg.thr + first, t.data(), sizeof(uint64_t) * t.size(), hipMemcpyHostToDevice, s));
        /* a new threshold is a new stream: the slots' segment state restarts */
        HIPCHK(hipMemsetAsync(b->sg.st + first, 0, sizeof(SgState) * (size_t)n, s));
        return MP3D_OK;
    });
}

/* The segment stage on stream s: dsmp [n][sstride][channels] samples and dcin
 * [n] counts are device memory; seg and seg_count are the caller's (host or
 * device).  Returns after the work is queued when both are device memory,
 * else when it is done. */
static int sg_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n, long long *seg,
                  long long seg_stride, int *seg_count, int flags, hipStream_t s) {
    mp3d_batch::SegmentSink &k = b->sg;
    const bool out_dev = is_device_ptr(seg, b->device);
    if (out_dev && (uintptr_t)seg % sizeof(long long)) return MP3D_E_ARG;
    CallerOut<int32_t> cnt;
    RCCHK(cnt.pick(b, (int32_t *)seg_count, k.cnt));
    /* no call emits more than the bound; a word of activity bits per tile of the hops it can touch */
    const long long stride = std::min(seg_stride, sg_bound(k.H, sstride, k.P, k.S));
    const long long tiles = std::max<long long>(1, (sg_hops(k.H, sstride) + MP3D_SG_TILE - 1) / MP3D_SG_TILE);
    /* one block per (stream, tile): the grid's blocks fit int and its threads 32 bits */
    if (tiles * n > 0x7fffffffLL || tiles * n * MP3D_SG_THREADS > 0xffffffffLL) return MP3D_E_CAPACITY;
    RCCHK(k.bits.grow(b, sizeof(uint64_t) * (size_t)n * (size_t)tiles));
    if (!out_dev) RCCHK(k.out.grow(b, 2 * sizeof(long long) * (size_t)stride * n + 16));
    long long *dout = out_dev ? seg : (long long *)k.out.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_segments(dsmp, dcin, k.st, k.plan, k.thr, k.part, k.bits, dout, cnt.dev, b->rs.ch, n, sstride,
                        out_dev ? seg_stride : stride, (int)tiles, k.H, k.P, k.S, k.pad,
                        (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    return deliver_rows(s, n, 2 * sizeof(long long), dout, stride, seg, seg_stride, cnt.dev, seg_count, out_dev,
                        !cnt.host);
}

extern "C" int mp3d_batch_segments(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts,
                                   int n, long long *seg, long long seg_stride, int *seg_count, int flags,
                                   void *hip_stream) {
    if (!b || !b->sg.on || !counts || !seg || !seg_count || sample_stride < 0 || seg_stride < 0 ||
        (flags & ~MP3D_PACK_FLUSH))
        return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > SG_MAX_STRIDE || seg_stride > 0x7fffffffLL) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp;
    const int32_t *dcin;
    bool host_in = false;
    RCCHK(stage_inputs(b, b->sg, samples, sample_stride, sizeof(float) * b->rs.ch, counts, n, s, &dsmp, &dcin,
                       &host_in));
    RCCHK(sg_run(b, dsmp, dcin, sample_stride, n, seg, seg_stride, seg_count, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_decode_segments(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                          const uint32_t *sizes, int n, int F, long long *seg, long long seg_stride,
                                          int *seg_count, int flags, mp3d_frame_info *infos, void *hip_stream) {
    if (!b || !b->sg.on || !seg || !seg_count || seg_stride < 0 || seg_stride > 0x7fffffffLL) return MP3D_E_ARG;
    long long S;
    hipStream_t s;
    RCCHK(decode_to_stage(b, b->sg, frames, offsets, sizes, n, F, flags, infos, hip_stream, &S, &s));
    CallEnd done{b, s};
    return sg_run(b, b->sg.smp, b->sg.cin, S, n, seg, seg_stride, seg_count, flags, s);
}

extern "C" int mp3d_batch_segment_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->sg.tm, us) : MP3D_E_ARG;
}
