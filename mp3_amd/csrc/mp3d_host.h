/*
 * mp3d_host.h -- private to the host sources (mp3d_host_tables.cpp,
 * mp3d_batch.cpp, mp3d_long.cpp, mp3d_dec.cpp, mp3d_sinks.cpp,
 * mp3d_loudness.cpp, mp3d_normalize.cpp, mp3d_stretch.cpp, mp3d_limiter.cpp): the error
 * macro, the owning device buffer, the batch handle and the internal
 * functions that cross those files.  Nothing here is exported (the library
 * is built with hidden visibility; the C ABI is include/mp3d.h).
 */
#ifndef MP3D_HOST_H
#define MP3D_HOST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/mp3d.h"
#include "mp3d_internal.h"
#include "mp3d_tables.h"
#include "mp3d_hostparse.h"
#include "mp3d_resample.h"
#include "mp3d_features.h"
#include "mp3d_loudness.h"
#include "mp3d_normalize.h"
#include "mp3d_stretch.h"
#include "mp3d_limiter.h"
#include "mp3d_launch.h"

namespace mp3d {

/* a HIP status as an MP3D_* code; a failure is kept for mp3d_last_hip_error */
inline thread_local int g_last_hip = 0;
inline int hip_rc(hipError_t e) {
    if (e == hipSuccess) return MP3D_OK;
    g_last_hip = (int)e;
    return e == hipErrorOutOfMemory ? MP3D_E_NOMEM : MP3D_E_HIP;
}
#define HIPCHK(x)                                                                                                      \
    do {                                                                                                               \
        if (const int _rc = mp3d::hip_rc(x)) return _rc;                                                               \
    } while (0)

/* per-device one-time init: constant symbols + table buffer (mp3d_host_tables.cpp) */
struct DeviceCtx {
    bool ready = false;
    DevTables *tables = nullptr;
    int n_cu = 256;
};
extern DeviceCtx g_dev[64];
int device_init(int device);

/* MP3D_DEBUG_POISON=1 at create: every device and
 * pinned allocation of the handle is filled with 0xFF when it is made, at
 * create and at every grow(), before the zeroing the code does on purpose.
 * A read of bytes nobody wrote then sees NaNs / huge lengths / all-ones
 * words on EVERY run, instead of whatever an earlier allocation left --
 * tests/test_gpu_poison.py runs the read-ahead, state and golden suites so. */
inline int poison_dev(bool on, void *p, size_t bytes, hipStream_t s) {
    if (!on || !p || !bytes) return MP3D_OK;
    HIPCHK(hipMemsetAsync(p, 0xFF, bytes, s));
    HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}
inline void poison_host(bool on, void *p, size_t bytes) {
    if (on && p) memset(p, 0xFF, bytes);
}

/* One device allocation and its size in bytes, freed with its owner.  The
 * owner waits for the work that uses it before it lets go. */
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { return std::swap(p, o.p), std::swap(cap, o.cap), *this; }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
    /* at least `need` bytes: a larger buffer replaces the old one (freed
     * first, never copied), poisoned when handle b's poison flag is on */
    int grow(const mp3d_batch *b, size_t need);
    operator T *() const { return p; }
};

/* one timed stage of a call (mp3d_batch_set_timing): an event on each side */
struct StageTimer {
    hipEvent_t ev[2] = {};
    bool timed = false; /* ev hold a call's stage */
    hipError_t begin(hipStream_t s) { return hipEventRecord(ev[0], s); }
    hipError_t end(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev[1], s);
        timed = timed || e == hipSuccess;
        return e;
    }
    int elapsed_us(float *us) const {
        HIPCHK(hipEventSynchronize(ev[1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *us = ms * 1000.f;
        return MP3D_OK;
    }
};

/* the resampling filters of one output rate (one per input rate), on the
 * host and on the device; hz = 0: none */
struct RsFilters {
    int hz = 0;
    RsCfg cfg = {};
    DevBuf<RsCfg> dcfg;
    DevBuf<float> tab;
    /* design, upload on stream s and wait (mp3d_sinks.cpp) */
    int upload(const mp3d_batch *b, int out_hz, int out_channels, hipStream_t s);
    void off() {
        dcfg.release(), tab.release();
        hz = 0;
    }
};

} // namespace mp3d

struct mp3d_batch {
    int device = 0, max_streams = 0, max_frames = 0;
    hipStream_t own = nullptr;
    bool poison = false; /* MP3D_DEBUG_POISON at create */
    /* the per-stream state the kernels use: st_mem, except while a long
     * decode runs its segments on scratch states (mp3d_long.cpp LongRun) */
    StreamState *st = nullptr;
    mp3d::DevBuf<StreamState> st_mem;
    mp3d::DevBuf<FrameRec> rec;
    mp3d::DevBuf<uint64_t> sideu; /* per-unit side info (k_demux -> k_huffman) */
    mp3d::DevBuf<int16_t> is_buf;
    mp3d::DevBuf<uint32_t> rank; /* k_rank: the units in big_values order per segment */
    mp3d::DevBuf<UnitMeta> meta;
    /* Stream geometry of a call (input offsets, sizes, md-region offsets) in
     * two device slots, each filled from its own pinned host buffer by an
     * async copy on the handle's copy stream: a call with new geometry (a
     * streaming loop's offsets advance every call) stages it and returns
     * without waiting; the copy overlaps the previous call's kernels.
     * Layout per slot for a call of n streams: in_off[n] u64, md_off[n] u64,
     * in_len[n] u32. */
    struct Geo {
        mp3d::DevBuf<uint64_t> d;
        uint64_t *h = nullptr;       /* pinned */
        hipEvent_t staged = nullptr; /* the copy h -> d is complete        */
        hipEvent_t freed = nullptr;  /* the last kernel reading d is done */
        bool fresh = false;          /* freed recorded by the slot's last reader */
        int n = -1;
        uint64_t *in_off() const { return d; }
        uint64_t *md_off() const { return d + n; }
        uint32_t *in_len() const { return (uint32_t *)(d + 2 * (size_t)n); }
    } geo[2];
    int geo_i = 0;
    /* d_work[0]: k_huffman's super-chunk counter (device; reset by each
     * launch's memset on the call's stream, and a handle's calls are
     * ordered).  d_work[1]: the family word, = call_seq when k_walk saw an
     * LSF stream in this call (fam_ok: this call's demux was k_walk) */
    mp3d::DevBuf<uint32_t> d_work;
    uint32_t call_seq = 0;
    bool fam_ok = false;
    hipStream_t copy = nullptr;
    mp3d::DevBuf<mp3d_frame_info> d_infos;
    mp3d::DevBuf<uint8_t> md;
    mp3d::DevBuf<uint8_t> d_in;   /* staging for host input */
    mp3d::DevBuf<int16_t> d_pcm;  /* staging for host output */
    mp3d::DevBuf<uint8_t> d_xr;   /* synth_only's staged spectra, block types and mixed flags */
    /* segmented synth-only calls: the final overlap + fifo per stream go to
     * a packed tail (the first segment may still be reading the state), and
     * the next synth-only call reads them from there: two tails used in
     * turn, so steady config-2 calls never copy state.  tail_live = the tail
     * holding streams [0, tail_n)'s current overlap + fifo (-1: StreamState
     * does); any other use of the handle first copies it back (flush_tail). */
    mp3d::DevBuf<float> st_tail[2];
    int tail_live = -1, tail_n = 0;
    bool timing = false;
    int opts = 0; /* MP3D_OPT_* */
    /* End of the handle's last call when it ran on a caller's stream,
     * recorded on that stream: sync, reset and state copies wait on this
     * event, never on the caller's stream handle (which the caller may have
     * destroyed since), and a call on another stream is ordered after it.
     * Calls on the handle's own stream (the per-frame decoder) record
     * nothing: own-stream order covers them. */
    hipEvent_t ev_done = nullptr;
    hipStream_t last_s = nullptr; /* compared with the next call's, never used */
    hipEvent_t ev[4] = {};
    /* packed PCM sink (mp3d_batch_set_output; mp3d_resample.h): f.hz = 0 is
     * off, and then none of these buffers exists.  st, plan, cnt hold
     * max_streams entries; rows (the float32 rows of a packed call), prefix
     * and out (staging for a host sink) grow with the calls. */
    struct PackedSink {
        mp3d::RsFilters f;
        int ch = 0;
        mp3d::DevBuf<RsState> st;
        mp3d::DevBuf<RsPlan> plan;
        mp3d::DevBuf<int32_t> cnt, prefix;
        mp3d::DevBuf<float> rows;
        mp3d::DevBuf<void> out;
        mp3d::StageTimer tm;
        void off() {
            f.off(), st.release(), plan.release(), cnt.release(), prefix.release(), rows.release(), out.release();
            ch = 0;
            tm.timed = false;
        }
    } rs;
    /* mp3d_batch_decode_long_packed to a rate other than the sink's: the
     * filters of its last output rate, kept for the next call */
    mp3d::RsFilters lp;
    /* log-mel feature sink (mp3d_batch_set_features; mp3d_features.h):
     * mels = 0 is off, and then none of these buffers exists.  st, plan, cin
     * (sample counts of a call) and cnt hold max_streams entries; smp (the
     * samples of a call) and out (staging for a host sink) grow with the
     * calls. */
    struct FeatureSink {
        int mels = 0;
        mp3d::DevBuf<FtTab> tab;
        mp3d::DevBuf<FtState> st;
        mp3d::DevBuf<FtPlan> plan;
        mp3d::DevBuf<int32_t> cin, cnt;
        mp3d::DevBuf<float> smp, out;
        mp3d::StageTimer tm;
        void off() {
            tab.release(), st.release(), plan.release(), cin.release(), cnt.release(), smp.release(), out.release();
            mels = 0;
            tm.timed = false;
        }
    } ft;
    /* loudness sink (mp3d_batch_set_loudness; mp3d_loudness.h): on = false is
     * off, and then none of these buffers exists.  st, plan, cin, cnt, pk, lu
     * (integrated loudness of a call's rows) and endst hold max_streams
     * entries; smp, out (staging for a host sink) and the per-tile scratch
     * tz, entry, part, tpeak grow with the calls. */
    struct LoudnessSink {
        bool on = false;
        int H = 0;
        mp3d::DevBuf<LdTab> tab;
        mp3d::DevBuf<LdState> st;
        mp3d::DevBuf<LdPlan> plan;
        mp3d::DevBuf<int32_t> cin, cnt;
        mp3d::DevBuf<float> smp, out, pk, lu, tpeak;
        mp3d::DevBuf<double> tz, entry, part, endst;
        mp3d::StageTimer tm;
        void off() {
            tab.release(), st.release(), plan.release(), cin.release(), cnt.release(), smp.release(), out.release();
            pk.release(), lu.release(), tpeak.release(), tz.release(), entry.release(), part.release(), endst.release();
            on = false, H = 0;
            tm.timed = false;
        }
    } ld;
    /* true-peak tap and gain (mp3d_batch_set_true_peak; mp3d_normalize.h):
     * on = false is off, and then taps, st and plan do not exist.  st, plan,
     * cin, tp hold max_streams entries; smp (a host caller's samples) and the
     * per-tile scratch tile grow with the calls.  The gain calls need only a
     * packed format: their staging (lu, gtp, gain for host arrays of the gain
     * rule; ccnt, gsmp, gcin, gg, out of mp3d_batch_apply_gain) is made by the
     * first call that needs it and freed with the packed format. */
    struct NormalizeSink {
        bool on = false;
        mp3d::DevBuf<float> taps;
        mp3d::DevBuf<TpState> st;
        mp3d::DevBuf<TpPlan> plan;
        mp3d::DevBuf<int32_t> cin, ccnt, gcin;
        mp3d::DevBuf<float> smp, tile, tp, lu, gtp, gain, gsmp, gg;
        mp3d::DevBuf<void> out;
        mp3d::StageTimer tm;
        /* the tap: the gain calls' staging stays */
        void tap_off() {
            taps.release(), st.release(), plan.release(), cin.release(), smp.release(), tile.release(), tp.release();
            on = false;
            tm.timed = false;
        }
        void off() {
            tap_off();
            ccnt.release(), gcin.release(), lu.release(), gtp.release(), gain.release(), gsmp.release(), gg.release();
            out.release();
        }
    } nm;
    /* tempo sink (mp3d_batch_set_stretch; mp3d_stretch.h): on = false is off,
     * and then none of these buffers exists.  st, plan, tempo (num, den per
     * slot; it outlives a restart of st), cin and cnt hold max_streams
     * entries; smp (a host caller's samples, or the packed samples of
     * mp3d_batch_decode_stretched) and out (staging for a host sink) grow with
     * the calls. */
    struct StretchSink {
        bool on = false;
        int H = 0;
        mp3d::DevBuf<float> w;
        mp3d::DevBuf<StState> st;
        mp3d::DevBuf<StPlan> plan;
        mp3d::DevBuf<int32_t> tempo, cin, cnt;
        mp3d::DevBuf<float> smp, out;
        mp3d::StageTimer tm;
        void off() {
            w.release(), st.release(), plan.release(), tempo.release(), cin.release(), cnt.release(), smp.release();
            out.release();
            on = false, H = 0;
            tm.timed = false;
        }
    } sx;
    /* limiter (mp3d_batch_set_limiter; mp3d_limiter.h): on = false is off, and
     * then none of these buffers exists.  taps, st, plan, cin, cnt, gg (a host
     * caller's gains) and grd (gr for a host caller) hold max_streams entries;
     * smp (a host caller's samples, or the packed samples of
     * mp3d_batch_decode_limited), out (staging for a host sink) and the
     * per-tile scratch tile grow with the calls. */
    struct LimiterSink {
        bool on = false;
        int A = 0;
        float c = 1.0f; /* the ceiling, linear */
        mp3d::DevBuf<float> taps;
        mp3d::DevBuf<LimState> st;
        mp3d::DevBuf<LimPlan> plan;
        mp3d::DevBuf<int32_t> cin, cnt;
        mp3d::DevBuf<float> smp, gg, grd, tile;
        mp3d::DevBuf<void> out;
        mp3d::StageTimer tm;
        void off() {
            taps.release(), st.release(), plan.release(), cin.release(), cnt.release(), smp.release(), gg.release();
            grd.release(), tile.release(), out.release();
            on = false, A = 0, c = 1.0f;
            tm.timed = false;
        }
    } lm;
};

namespace mp3d {

template <class T> int DevBuf<T>::grow(const mp3d_batch *b, size_t need) {
    if (need <= cap) return MP3D_OK;
    if (p) HIPCHK(hipFree(p));
    p = nullptr, cap = 0;
    HIPCHK(hipMalloc((void **)&p, need));
    cap = need;
    return poison_dev(b->poison, p, need, b->own);
}

/* an event after all of the handle's work issued so far */
inline hipEvent_t end_event(mp3d_batch *b) {
    if (!b->last_s || b->last_s == b->own) (void)hipEventRecord(b->ev_done, b->own);
    return b->ev_done;
}

/* a call on stream s: order it after the handle's previous call (the
 * handle's buffers are shared).  Only two calls in a row on the handle's own
 * stream skip the wait; after a call on a caller's stream the wait is made
 * even when s compares equal, since a destroyed stream's handle value can be
 * reused by the caller's next stream (a no-op once the event completed). */
inline int call_begin(mp3d_batch *b, hipStream_t s) {
    HIPCHK(hipSetDevice(b->device));
    if (b->last_s && (b->last_s != s || s != b->own)) HIPCHK(hipStreamWaitEvent(s, end_event(b), 0));
    return MP3D_OK;
}

/* the own stream (sync, reset, state copies) after the handle's last call */
inline int own_after_last(mp3d_batch *b) {
    if (b->last_s && b->last_s != b->own) HIPCHK(hipStreamWaitEvent(b->own, b->ev_done, 0));
    return MP3D_OK;
}

/* when a public call returns: ev_done on a caller's stream */
struct CallEnd {
    mp3d_batch *b;
    hipStream_t s;
    ~CallEnd() {
        if (s == b->own || hipEventRecord(b->ev_done, s) == hipSuccess) b->last_s = s;
    }
};

/* ---- mp3d_batch.cpp ---- */
/* Where a caller's buffer lives, seen from the handle's device: its own
 * device memory (or managed memory) is read and written in place by the
 * kernels; host memory and another GPU's memory are staged through the
 * handle's buffers with hipMemcpyDefault copies (no peer access assumed). */
enum PtrKind { PTR_HOST, PTR_DEV, PTR_OTHER_DEV };
PtrKind ptr_kind(const void *p, int device);
/* memory the handle's kernels may read / write in place */
inline bool is_device_ptr(const void *p, int device) { return ptr_kind(p, device) == PTR_DEV; }
/* StreamState slots [0, n) zeroed with their format stamp, on stream s (the
 * caller orders / waits) */
hipError_t state_clear(StreamState *st, int n, hipStream_t s);
/* the live tail back into StreamState (on stream s) */
int flush_tail(mp3d_batch *b, hipStream_t s);
/* a state blob's format stamps checked before anything is written */
int blob_check(mp3d_batch *b, int n, const void *src);
int prepare_geometry(mp3d_batch *b, const uint64_t *offsets, const uint32_t *sizes, int n, hipStream_t s);

/* One run of pre-located, complete frames of one stream (the per-frame
 * decoder's read-ahead, mp3d_dec.cpp ra_fill): the bytes and the frame
 * offsets in mapped host memory, read by k_demux_fp directly (no copy); the
 * previous run's synthesis tail flushed and the state snapshot taken inside
 * that kernel; no stream geometry to stage (one stream at md offset 0).  A
 * run costs three kernel launches and no copy. */
struct FpRun {
    const uint8_t *in;   /* device address of the run's bytes (mapped)    */
    uint32_t len;
    const uint32_t *fo;  /* the frame offsets (host; passed as kernel arguments) */
    const float *tail_in; /* the handle's live synthesis tail, or null     */
    StreamState *snap;   /* receives the state before the run             */
};
/* decode into int16 (f32 = false) or float32 PCM, both [n][F][2304] */
/* kinds: k_synth family variants to launch (bit 0 MPEG-1, bit 1 LSF); 3 for
 * a batch, one bit for the per-frame decoder, which knows its frame's family */
/* mapped: frames, pcm and infos are device-accessible pinned host memory
 * (the per-frame decoder): the kernels read and write them in place and the
 * call ends with one stream sync */
/* async (mapped only): return without waiting; the caller records an event */
int batch_decode(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets, const uint32_t *sizes, int n, int F,
                 void *pcm, bool f32, mp3d_frame_info *infos, void *hip_stream, bool overwrite, int kinds = 3,
                 bool mapped = false, int seg_len_req = 0, const FpRun *fp = nullptr, bool async = false);

/* ---- mp3d_sinks.cpp ---- */
extern const int RS_RATES[MP3D_RS_RATES];
int rs_rate_index(int hz); /* -1: not an MPEG audio rate */
/* interpolation L, decimation M and taps per phase T of one rate pair */
void rs_sizes(int in_hz, int out_hz, int *L, int *M, int *T);
/* the most outputs one call of `frames` frames at in_hz can emit: all its
 * inputs plus a pending tail of `post` inputs, ceil((N + post) L / M) */
long long rs_bound(int in_hz, int out_hz, long long frames);
/* The tail of a sink call on stream s: n streams' rows (`unit` bytes each)
 * and counts reach the caller.  drows [n][dstride] and dcnt [n] are where
 * the kernels put them: the caller's own memory when rows_dev / cnt_dev
 * (nothing to do for that part), else the handle's staging, and then only
 * each stream's own rows are copied to the caller's rows [n][stride].
 * Returns after the work is queued when both are device memory, else when
 * it is done. */
int deliver_rows(hipStream_t s, int n, size_t unit, const void *drows, long long dstride, void *rows, long long stride,
                 const int32_t *dcnt, int *count, bool rows_dev, bool cnt_dev);

} // namespace mp3d

#endif
