/*
 * mp3d_host.h -- private to the host sources (mp3d_host_tables.cpp,
 * mp3d_batch.cpp, mp3d_long.cpp, mp3d_dec.cpp, mp3d_sinks.cpp,
 * mp3d_loudness.cpp, mp3d_normalize.cpp, mp3d_stretch.cpp, mp3d_limiter.cpp,
 * mp3d_segment.cpp, mp3d_eq.cpp, mp3d_pitch.cpp):
 * the error macros, the readers of the environment's knobs, the owning types
 * (DevBuf device memory, PinBuf pinned host memory, Event), the batch handle,
 * the frame that every call shares -- the core decode (DecodeCall,
 * core_launch), the long-stream calls, the per-frame decoder and the stages
 * behind the packed sink (stage_launch, set_begin / set_end, CallerOut,
 * CallEnd) -- and the internal functions that cross those files.  Nothing
 * here is exported (the library is built with hidden visibility; the C ABI is
 * include/mp3d.h).
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
#include "mp3d_segment.h"
#include "mp3d_eq.h"
#include "mp3d_pitch.h"
#include "mp3d_launch.h"

namespace mp3d {

/* a HIP status as an MP3D_* code; a failure is kept for mp3d_last_hip_error */
inline thread_local int g_last_hip = 0;
inline int hip_rc(hipError_t e) {
    if (e == hipSuccess) return MP3D_OK;
    g_last_hip = (int)e;
    return e == hipErrorOutOfMemory ? MP3D_E_NOMEM : MP3D_E_HIP;
}
/* return an MP3D_* failure (RCCHK) or a HIP one (HIPCHK) to the caller */
#define RCCHK(x)                                                                                                       \
    do {                                                                                                               \
        if (const int _rc = (x)) return _rc;                                                                           \
    } while (0)
#define HIPCHK(x) RCCHK(mp3d::hip_rc(x))

/* The environment's knobs are read through these four and nowhere else.
 * env_set: set to anything, the empty word included; env_flag: set and
 * neither empty nor "0"; env_is: set to this word; env_int: an integer
 * (atoi) clamped to [lo, hi], dflt when unset. */
inline bool env_set(const char *name) { return getenv(name) != nullptr; }
inline bool env_flag(const char *name) {
    const char *e = getenv(name);
    return e && e[0] && strcmp(e, "0") != 0;
}
inline bool env_is(const char *name, const char *word) {
    const char *e = getenv(name);
    return e && !strcmp(e, word);
}
inline int env_int(const char *name, int dflt, int lo, int hi) {
    const char *e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : dflt;
}

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

/* One pinned host allocation, freed with its owner, and its device address
 * when it was mapped (m = null: the device reaches it through copies only). */
template <class T> struct PinBuf {
    T *p = nullptr, *m = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
    /* `bytes` with hipHostMalloc's `flags`, filled with 0xFF when `poison` */
    hipError_t alloc(size_t bytes, unsigned flags, bool poison) {
        const hipError_t e = hipHostMalloc((void **)&p, bytes, flags);
        poison_host(poison && e == hipSuccess, p, bytes);
        return e;
    }
    /* m = the device address; after a failure m is null */
    hipError_t map() {
        const hipError_t e = hipHostGetDevicePointer((void **)&m, p, 0);
        if (e != hipSuccess) m = nullptr;
        return e;
    }
    operator T *() const { return p; }
};

/* One event, destroyed with its owner (after the owner's waits).  An
 * ordering event is made by create() when its owner is; a timing event is
 * made by the first record_timed(), so a handle that never times has none
 * and a failed creation is the error of the call that needed the event. */
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e, flags); }
    hipError_t record_timed(hipStream_t s) {
        if (!e) {
            const hipError_t r = create(hipEventDefault);
            if (r != hipSuccess) return r;
        }
        return hipEventRecord(e, s);
    }
    operator hipEvent_t() const { return e; }
};

/* one timed stage of a call (mp3d_batch_set_timing): an event on each side */
struct StageTimer {
    Event ev[2];
    bool timed = false; /* ev hold a call's stage */
    hipError_t begin(hipStream_t s) { return ev[0].record_timed(s); }
    hipError_t end(hipStream_t s) {
        const hipError_t e = ev[1].record_timed(s);
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
        mp3d::PinBuf<uint64_t> h;
        mp3d::Event staged; /* the copy h -> d is complete        */
        mp3d::Event freed;  /* the last kernel reading d is done */
        bool fresh = false; /* freed recorded by the slot's last reader */
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
    mp3d::Event ev_done;
    hipStream_t last_s = nullptr; /* compared with the next call's, never used */
    /* the core decode's timing (mp3d_batch_kernel_times), a chain on the
     * call's stream: before demux, after demux, after Huffman, after
     * synthesis (core_mark, core_launch) */
    mp3d::Event ev[4];
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
    /* What every stage downstream of the packed sink has (DESIGN.md section
     * 4d): a call's inputs when they are not the caller's own device memory
     * (smp: a host caller's samples or the packed samples of the stage's
     * decode_* call; cin: their counts), staging for a host caller's outputs
     * (out: rows; cnt: their counts) and the stage's timer.  cin and cnt hold
     * max_streams entries; smp and out grow with the calls.  A stage leaves
     * what it does not use empty. */
    struct Stage {
        mp3d::DevBuf<float> smp;
        mp3d::DevBuf<int32_t> cin, cnt;
        mp3d::DevBuf<void> out;
        mp3d::StageTimer tm;
        void off() {
            smp.release(), cin.release(), cnt.release(), out.release();
            tm.timed = false;
        }
    };
    /* log-mel feature sink (mp3d_batch_set_features; mp3d_features.h):
     * mels = 0 is off, and then none of its buffers exists.  st and plan hold
     * max_streams entries. */
    struct FeatureSink : Stage {
        int mels = 0;
        mp3d::DevBuf<FtTab> tab;
        mp3d::DevBuf<FtState> st;
        mp3d::DevBuf<FtPlan> plan;
        void off() {
            Stage::off(), tab.release(), st.release(), plan.release();
            mels = 0;
        }
    } ft;
    /* loudness sink (mp3d_batch_set_loudness; mp3d_loudness.h): on = false is
     * off, and then none of its buffers exists.  st, plan, pk, lu (integrated
     * loudness of a call's rows) and endst hold max_streams entries; the
     * per-tile scratch tz, entry, part, tpeak grows with the calls. */
    struct LoudnessSink : Stage {
        bool on = false;
        int H = 0;
        mp3d::DevBuf<LdTab> tab;
        mp3d::DevBuf<LdState> st;
        mp3d::DevBuf<LdPlan> plan;
        mp3d::DevBuf<float> pk, lu, tpeak;
        mp3d::DevBuf<double> tz, entry, part, endst;
        void off() {
            Stage::off(), tab.release(), st.release(), plan.release(), pk.release(), lu.release(), tpeak.release();
            tz.release(), entry.release(), part.release(), endst.release();
            on = false, H = 0;
        }
    } ld;
    /* true-peak tap (mp3d_batch_set_true_peak; mp3d_normalize.h): on = false
     * is off, and then none of its buffers exists.  st, plan and tp hold
     * max_streams entries; the per-tile scratch tile grows with the calls. */
    struct TruePeakTap : Stage {
        bool on = false;
        mp3d::DevBuf<float> taps, tile, tp;
        mp3d::DevBuf<TpState> st;
        mp3d::DevBuf<TpPlan> plan;
        void off() {
            Stage::off(), taps.release(), tile.release(), tp.release(), st.release(), plan.release();
            on = false;
        }
    } nm;
    /* The gain calls (mp3d_batch_normalize_gain, mp3d_batch_apply_gain) need
     * only a packed format: their staging (lu, gtp, gain for host arrays of
     * the gain rule; smp, cin, gg, out and the clamped counts cnt of
     * mp3d_batch_apply_gain) is made by the first call that needs it and
     * freed with the packed format. */
    struct GainCalls : Stage {
        mp3d::DevBuf<float> lu, gtp, gain, gg;
        void off() { Stage::off(), lu.release(), gtp.release(), gain.release(), gg.release(); }
    } ga;
    /* tempo sink (mp3d_batch_set_stretch; mp3d_stretch.h): on = false is off,
     * and then none of its buffers exists.  st, plan and tempo (num, den per
     * slot; it outlives a restart of st) hold max_streams entries. */
    struct StretchSink : Stage {
        bool on = false;
        int H = 0;
        mp3d::DevBuf<float> w;
        mp3d::DevBuf<StState> st;
        mp3d::DevBuf<StPlan> plan;
        mp3d::DevBuf<int32_t> tempo;
        void off() {
            Stage::off(), w.release(), st.release(), plan.release(), tempo.release();
            on = false, H = 0;
        }
    } sx;
    /* limiter (mp3d_batch_set_limiter; mp3d_limiter.h): on = false is off, and
     * then none of its buffers exists.  taps, st, plan, gg (a host caller's
     * gains) and grd (gr for a host caller) hold max_streams entries; the
     * per-tile scratch tile grows with the calls. */
    struct LimiterSink : Stage {
        bool on = false;
        int A = 0;
        float c = 1.0f; /* the ceiling, linear */
        mp3d::DevBuf<float> taps, gg, grd, tile;
        mp3d::DevBuf<LimState> st;
        mp3d::DevBuf<LimPlan> plan;
        void off() {
            Stage::off(), taps.release(), gg.release(), grd.release(), tile.release(), st.release(), plan.release();
            on = false, A = 0, c = 1.0f;
        }
    } lm;
    /* segment sink (mp3d_batch_set_segments; mp3d_segment.h): on = false is
     * off, and then none of its buffers exists.  st, plan, thr (it outlives a
     * restart of st) and part hold max_streams entries; the per-tile activity
     * words bits grow with the calls. */
    struct SegmentSink : Stage {
        bool on = false;
        int H = 0, P = 0, S = 0, pad = 0; /* the hop in samples; pause, shortest segment and pad in hops */
        mp3d::DevBuf<SgState> st;
        mp3d::DevBuf<SgPlan> plan;
        mp3d::DevBuf<uint64_t> thr, part, bits;
        void off() {
            Stage::off(), st.release(), plan.release(), thr.release(), part.release(), bits.release();
            on = false, H = P = S = pad = 0;
        }
    } sg;
    /* equaliser (mp3d_batch_set_eq; mp3d_eq.h): K = 0 is off, and then none of
     * its buffers exists.  st and plan hold max_streams entries, tab and tpow
     * the curve's constants; the per-tile scratch tz, entry grows with the
     * calls. */
    struct EqSink : Stage {
        int K = 0; /* sections of the curve */
        mp3d::DevBuf<EqTab> tab;
        mp3d::DevBuf<double> tpow, tz, entry;
        mp3d::DevBuf<EqState> st;
        mp3d::DevBuf<EqPlan> plan;
        void off() {
            Stage::off(), tab.release(), tpow.release(), tz.release(), entry.release(), st.release(), plan.release();
            K = 0;
        }
    } eq;
    /* pitch sink (mp3d_batch_set_pitch; mp3d_pitch.h): on = false is off, and
     * then none of its buffers exists.  st and plan hold max_streams entries. */
    struct PitchSink : Stage {
        bool on = false;
        int H = 0, T = 0, tmin = 0, theta = 0; /* the hop, tmax + 1 and tmin in samples; the threshold in 1/1024 */
        mp3d::DevBuf<PtState> st;
        mp3d::DevBuf<PtPlan> plan;
        void off() {
            Stage::off(), st.release(), plan.release();
            on = false, H = T = tmin = theta = 0;
        }
    } pt;
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

/* Where a caller's buffer lives, seen from the handle's device: its own
 * device memory (or managed memory) is read and written in place by the
 * kernels; host memory and another GPU's memory are staged through the
 * handle's buffers with hipMemcpyDefault copies (no peer access assumed).
 * (mp3d_batch.cpp) */
enum PtrKind { PTR_HOST, PTR_DEV, PTR_OTHER_DEV };
PtrKind ptr_kind(const void *p, int device);
/* memory the handle's kernels may read / write in place */
inline bool is_device_ptr(const void *p, int device) { return ptr_kind(p, device) == PTR_DEV; }

/* The stages downstream of the packed sink, listed once. A new sink adds its
 * line to stages_off and to stages_restart; nothing else names them all (a
 * stage's timer owns its events). */
/* they read the packed sink's format: off with any change of it */
inline void stages_off(mp3d_batch *b) {
    b->ft.off(), b->ld.off(), b->nm.off(), b->ga.off(), b->sx.off(), b->lm.off(), b->sg.off(), b->eq.off(), b->pt.off();
}
template <class S> hipError_t stage_restart(const DevBuf<S> &st, int first, int n, hipStream_t s) {
    return st ? hipMemsetAsync(st + first, 0, sizeof(S) * (size_t)n, s) : hipSuccess;
}
/* slots [first, first + n) of every stage that is on start a new stream, on stream s */
inline int stages_restart(mp3d_batch *b, int first, int n, hipStream_t s) {
    HIPCHK(stage_restart(b->ft.st, first, n, s));
    HIPCHK(stage_restart(b->ld.st, first, n, s));
    HIPCHK(stage_restart(b->nm.st, first, n, s));
    HIPCHK(stage_restart(b->sx.st, first, n, s));
    HIPCHK(stage_restart(b->lm.st, first, n, s));
    HIPCHK(stage_restart(b->sg.st, first, n, s));
    HIPCHK(stage_restart(b->eq.st, first, n, s));
    HIPCHK(stage_restart(b->pt.st, first, n, s));
    return MP3D_OK;
}

/* ---- the frame of a stage's calls, which the core
 * decode, the long-stream calls and the per-frame decoder use too ---- */
/* the head of a set_* call: the handle idle, its last call done */
inline int set_begin(mp3d_batch *b) {
    HIPCHK(hipSetDevice(b->device));
    RCCHK(own_after_last(b));
    HIPCHK(hipStreamSynchronize(b->own));
    return MP3D_OK;
}
/* its tail, r the result so far: the uploads waited for (they read the
 * caller's stack), and after a failure stage k is off */
template <class K> int set_end(mp3d_batch *b, K &k, int r) {
    if (!r) r = hip_rc(hipStreamSynchronize(b->own));
    if (r) k.off();
    k.tm.timed = false;
    return r;
}

/* One launch of a stage on stream s: between the timer's events when the
 * handle times its stages (tm = null: an untimed small kernel), after the
 * LDS poison when the handle poisons */
template <class F> int stage_launch(mp3d_batch *b, StageTimer *tm, hipStream_t s, F &&launch) {
    if (!b->timing) tm = nullptr;
    if (tm) HIPCHK(tm->begin(s));
    if (b->poison) launch_lds_poison(g_dev[b->device].n_cu, s);
    launch();
    if (tm) HIPCHK(tm->end(s));
    return hip_rc(hipGetLastError());
}

/* event i of the core decode's timing chain (mp3d_batch.ev) on stream s, when
 * the handle times */
inline int core_mark(mp3d_batch *b, int i, hipStream_t s) {
    if (b->timing) HIPCHK(b->ev[i].record_timed(s));
    return MP3D_OK;
}
/* One launch of the core decode on stream s, as a stage's, then event i of
 * the chain: the time from the event before it is this kernel's */
template <class F> int core_launch(mp3d_batch *b, int i, hipStream_t s, F &&launch) {
    RCCHK(stage_launch(b, nullptr, s, launch));
    return core_mark(b, i, s);
}

/* The tail the per-slot setters share (mp3d_batch_set_window, _set_tempo,
 * _set_segment_threshold), after a setter's own validation: the own stream
 * ordered after the handle's last call, on any stream; `queue(s)`, the
 * setter's copy of its parameters and restart of the slots' state, in the
 * setter's order; and the wait (the parameters are on the setter's stack). */
template <class F> int slots_set(mp3d_batch *b, F &&queue) {
    HIPCHK(hipSetDevice(b->device));
    RCCHK(own_after_last(b));
    RCCHK(queue(b->own));
    return hip_rc(hipStreamSynchronize(b->own));
}

/* behind the *_time exports */
inline int stage_time(const mp3d_batch *b, const StageTimer &tm, float *us) {
    if (!us || !b->timing || !tm.timed) return MP3D_E_ARG;
    return tm.elapsed_us(us);
}

/* A caller's n-element array (or null) for a kernel to read on stream s:
 * itself when it is device memory (element-aligned, else MP3D_E_ARG), else a
 * copy in `stage` (max_streams elements); *host is set when the caller's host
 * memory is read, until the stream reaches the copy's end */
template <class T>
int caller_in(mp3d_batch *b, const T *p, int n, DevBuf<T> &stage, hipStream_t s, const T **dev, bool *host) {
    *dev = p;
    if (!p) return MP3D_OK;
    if (is_device_ptr(p, b->device)) return (uintptr_t)p % sizeof(T) ? MP3D_E_ARG : MP3D_OK;
    RCCHK(stage.grow(b, sizeof(T) * (size_t)b->max_streams));
    HIPCHK(hipMemcpyAsync(stage.p, p, sizeof(T) * (size_t)n, hipMemcpyDefault, s));
    *dev = stage.p;
    *host = true;
    return MP3D_OK;
}

/* A caller's n-element array (or null) for a kernel to write: dev is the
 * array itself when it is device memory (element-aligned, else MP3D_E_ARG),
 * else `stage` (max_streams elements), and then copy_back queues the copy to
 * the caller after the kernel; the caller of copy_back waits. */
template <class T> struct CallerOut {
    T *user = nullptr, *dev = nullptr;
    bool host = false; /* dev is the staging */
    int pick(mp3d_batch *b, T *p, DevBuf<T> &stage) {
        user = dev = p;
        if (!p) return MP3D_OK;
        if (is_device_ptr(p, b->device)) return (uintptr_t)p % sizeof(T) ? MP3D_E_ARG : MP3D_OK;
        RCCHK(stage.grow(b, sizeof(T) * (size_t)b->max_streams));
        dev = stage.p;
        host = true;
        return MP3D_OK;
    }
    hipError_t copy_back(int n, hipStream_t s) const {
        return host ? hipMemcpyAsync(user, dev, sizeof(T) * (size_t)n, hipMemcpyDefault, s) : hipSuccess;
    }
};

/* ---- mp3d_batch.cpp ---- */
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
/* One call of the core decode (demux, Huffman, synthesis), filled by field
 * name: the public decodes leave the options at their defaults. */
struct DecodeCall {
    /* input: stream i is sizes[i] bytes at frames + offsets[i]; n streams, F frames of each */
    const uint8_t *frames = nullptr;
    const uint64_t *offsets = nullptr;
    const uint32_t *sizes = nullptr;
    int n = 0, F = 0;
    /* sink: PCM [n][F][2304], int16 or (f32) float32; frame infos [n][F] or
     * null; the caller's stream, or null for the handle's own */
    void *pcm = nullptr;
    bool f32 = false;
    mp3d_frame_info *infos = nullptr;
    void *hip_stream = nullptr;
    /* A host PCM buffer is read back whole.  false: the bytes the kernels
     * did not write (rows without audio, the second half of a mono / LSF
     * row) are saved from the caller's buffer first and put back; true: they
     * are not (an internal caller that reads only the rows' audio). */
    bool clobber_unwritten = false;
    /* k_synth family variants to launch (bit 0 MPEG-1, bit 1 LSF): 3 for a
     * batch, one bit for the per-frame decoder, which knows its frame's family */
    int kinds = 3;
    /* frames, pcm and infos are device-accessible pinned host memory (the
     * per-frame decoder): the kernels read and write them in place and the
     * call ends with one stream sync */
    bool mapped = false;
    /* frames per synthesis segment; 0: chosen from n and F */
    int seg_len = 0;
    /* the front half runs on these pre-located frames of one stream (then
     * frames, offsets and sizes are not read) */
    const FpRun *fp = nullptr;
    /* return without waiting (mapped only, else MP3D_E_ARG); the caller records an event */
    bool async = false;
};
int batch_decode(mp3d_batch *b, const DecodeCall &c);

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
/* The inputs of a stage's call on the caller's samples [n][stride] (`frame`
 * bytes per sample frame) and counts [n], for the kernels on stream s: each
 * is the caller's own when it is device memory (float- / int-aligned, else
 * MP3D_E_ARG), else a copy in k.smp / k.cin.  *host as in caller_in. */
int stage_inputs(mp3d_batch *b, mp3d_batch::Stage &k, const float *samples, long long stride, size_t frame,
                 const int *counts, int n, hipStream_t s, const float **dsmp, const int32_t **dcin, bool *host);
/* the stride of a decode_* call's packed samples: one no stream of F frames can exceed */
inline long long stage_stride(const mp3d_batch *b, int F) { return mp3d_packed_max_samples(b->rs.f.hz, F, 0); }
/* The head of a stage's decode_* call, after the wrapper's own checks: the
 * checks they share (argument errors before capacity errors), then the packed
 * call into the stage's own samples k.smp [n][*S] and counts k.cin, which only
 * queues work; *s is the call's stream. */
int decode_to_stage(mp3d_batch *b, mp3d_batch::Stage &k, const uint8_t *frames, const uint64_t *offsets,
                    const uint32_t *sizes, int n, int F, int flags, mp3d_frame_info *infos, void *hip_stream,
                    long long *S, hipStream_t *s);

} // namespace mp3d

#endif
