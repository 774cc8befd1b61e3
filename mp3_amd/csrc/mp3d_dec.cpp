/*
 * mp3d_dec.cpp -- the per-frame decoder of the C ABI (include/mp3d.h): a
 * one-stream batch plus pinned staging, so a call is one small DMA each way
 * and one stream sync, and its read-ahead.  The frame is staged zero-padded
 * to a fixed MP3D_PF_BYTES, which keeps the batch geometry constant
 * (uploaded once) across calls.
 */
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "mp3d_host.h"

using namespace mp3d;

#define MP3D_PF_BYTES 4096
#define MP3D_PF_READAHEAD 64 /* frames per read-ahead by default (k_demux_fp: <= 64) */
#define MP3D_PF_RA_SEG 1     /* synthesis segment (frames) of a read-ahead */
struct mp3d_dec {
    mp3d_batch *b = nullptr;
    long frames = 0;
    int kind = 0; /* MPEG family of the stream's first frame (StreamState.kind) */
    /* pinned, with their device addresses (.m) when mapped: the kernels read
     * the frame and write PCM + info in place, no copies (.m null: staged
     * copies instead) */
    PinBuf<uint8_t> in;           /* the frame, zero-padded */
    PinBuf<float> out;            /* one frame of PCM       */
    PinBuf<mp3d_frame_info> info; /* its frame info         */
    /* one-launch path (k_frame): the kernel writes the call's sequence
     * number into this mapped word after its PCM; the host polls it */
    PinBuf<uint32_t> done;
    uint32_t seq = 0;
    bool fused = false;
    /* Read-ahead: the player hands over the
     * rest of its buffer, so one call decodes up to ra_max of the frames
     * found there in ONE batch call (n = 1, F = ra_max; the host-located
     * frames demuxed frame-parallel by k_demux_fp, frame-parallel synthesis
     * segments) into mapped buffers, and the next calls are served from them
     * after checking that the caller's bytes at the located frame are the
     * same.  Two runs: while the calls are served from one, the next run
     * (the frames after it in the same buffer) decodes behind them, launched
     * without waiting, so a player's steady state never waits for a refill.
     * Any other input (a seek, a new buffer, other options or sink) settles
     * first: the state saved before the run being served is restored and
     * the frames already served are decoded again (exact), the next run is
     * dropped, then the call runs normally.  MP3D_PF_READAHEAD = frames per
     * run (0 / 1: off); MP3D_PF_RA_NEXT=0: no next run (one run at a time). */
    int ra_max = 0;
    int ra_seg = MP3D_PF_RA_SEG; /* MP3D_PF_RA_SEG env: synthesis segment of a read-ahead */
    bool ra_next_on = true;
    struct RaEnt {
        uint32_t off, len; /* the frame's bytes in the run's in buffer */
        size_t pos;        /* bytes skipped before it in its call's buffer */
    };
    struct Run {
        /* pinned, mapped.  in: frames back to back, then the u32 frame offsets;
         * k_demux_fp reads it in place (all frames at once, so one PCIe round
         * trip per phase, not one per frame) */
        PinBuf<uint8_t> in;
        PinBuf<uint8_t> pcm; /* [ra_max][2304] f32-sized slots */
        PinBuf<mp3d_frame_info> inf;
        DevBuf<StreamState> snap; /* device: the state before the run */
        Event done;               /* the run's batch call has completed */
        std::vector<RaEnt> ents;
        uint32_t fo_at = 0;           /* byte offset of the frame offsets in in / dev */
        bool f32 = false;
        bool pending = false;         /* launched without waiting (the next run) */
    } run[2];
    int cur = 0;       /* run[cur] is served; run[cur ^ 1] is the next run, if any */
    size_t ra_next = 0; /* next entry of run[cur] to serve */
    /* back-off: a settle that drops frames decoded ahead wasted
     * them, so the next ra_cool calls decode their own frame only; each such
     * settle doubles the pause (up to 64 calls), a read-ahead served whole
     * clears it.  A player that saves its state every frame then pays one
     * read-ahead per ~65 frames instead of two batch decodes per frame. */
    int ra_cool = 0, ra_backoff = 0;
    /* A read-ahead launch or settle that failed part-way may have advanced
     * the device state (k_demux_fp writes it and the snapshot first) with no
     * record of where to: every later call returns this error until
     * mp3d_dec_reset or a successful mp3d_dec_set_state. */
    std::atomic<int> broken{0}; /* (written by the helper thread, read by the caller's) */
    /* MP3D_DEBUG_RA_DELAY_US: the helper thread sleeps this long before each
     * launch (tests: the served calls must not depend on its timing) */
    int wk_delay_us = 0;
    /* MP3D_DEBUG_RA_FAIL=n: the n-th next-run launch reports MP3D_E_HIP after
     * its kernels were queued (the state then sits past the served frames) */
    int dbg_fail = 0, dbg_launches = 0;
    /* The next run's launch (its HIP calls: three kernel launches and an
     * event, tens of microseconds of host time) runs on a helper thread, so
     * the call that hands it over returns at once; the frames are staged
     * into the run's buffer by the calling thread first (the caller's buffer
     * is valid only during its call).  Every call that touches the batch
     * handle joins the helper first (ra_join); a call served from the
     * current run does not.  MP3D_PF_RA_THREAD=0: launch on the calling
     * thread. */
    bool wk_on = true;
    std::thread wk;
    std::mutex wk_mu;
    std::condition_variable wk_cv;
    bool wk_job = false, wk_quit = false;
    int wk_rc = 0;
    struct WkJob {
        Run *u;
        uint32_t o;
        int kinds;
        bool f32;
    } wk_arg{};
    mp3d_dec::Run &R() { return run[cur]; }
    mp3d_dec::Run &N() { return run[cur ^ 1]; }
};

static void dec_free(mp3d_dec *d) {
    if (d->wk.joinable()) {
        {
            std::lock_guard<std::mutex> lk(d->wk_mu);
            d->wk_quit = true;
        }
        d->wk_cv.notify_all();
        d->wk.join(); /* (after its last job) */
    }
    if (d->b) mp3d_batch_destroy(d->b); /* (waits for the handle's work, a next run included) */
    delete d;                           /* frees its pinned buffers and the runs' events */
}

static void ra_worker(mp3d_dec *d);
extern "C" int mp3d_dec_create_on(int device, mp3d_dec **out) {
    if (!out) return MP3D_E_ARG;
    *out = nullptr;
    mp3d_dec *d = new (std::nothrow) mp3d_dec;
    if (!d) return MP3D_E_NOMEM;
    const int imax = 0x7fffffff;
    d->ra_max = env_int("MP3D_PF_READAHEAD", MP3D_PF_READAHEAD, 0, 64);
    if (d->ra_max < 2) d->ra_max = 0;
    d->ra_seg = env_int("MP3D_PF_RA_SEG", MP3D_PF_RA_SEG, 1, imax);
    d->ra_next_on = !env_is("MP3D_PF_RA_NEXT", "0");
    d->wk_on = !env_is("MP3D_PF_RA_THREAD", "0");
    /* test hooks: the helper's launch delayed, the n-th next-run launch
     * failed after it ran (tests/test_gpu_poison.py) */
    d->wk_delay_us = env_int("MP3D_DEBUG_RA_DELAY_US", 0, 0, imax);
    d->dbg_fail = env_int("MP3D_DEBUG_RA_FAIL", 0, 0, imax);
    /* a failure from here on: everything made so far freed */
    auto fail = [d](int rc) {
        dec_free(d);
        return rc;
    };
    if (const int r = mp3d_batch_create(device, 1, std::max(1, d->ra_max), &d->b)) return fail(r);
    /* the buffers the device writes are coherent (not cached in the GPU's
     * L2), so the completion word's fence orders them for the host;
     * MP3D_DEBUG_POISON: the per-call pinned buffers too */
    const unsigned co = hipHostMallocMapped | hipHostMallocCoherent;
    const bool poison = d->b->poison;
    if (d->in.alloc(MP3D_PF_BYTES, hipHostMallocDefault, poison) != hipSuccess ||
        d->out.alloc(sizeof(float) * 2304, co, poison) != hipSuccess ||
        d->info.alloc(sizeof(mp3d_frame_info), co, poison) != hipSuccess ||
        d->done.alloc(64, co, false) != hipSuccess)
        return fail(MP3D_E_NOMEM);
    *d->done.p = 0u;
    if (!env_set("MP3D_PF_STAGED") && d->in.map() == hipSuccess && d->out.map() == hipSuccess &&
        d->info.map() == hipSuccess && d->done.map() == hipSuccess) {
        /* MP3D_PF_FUSED=0: the three-kernel path with a stream sync (tests
         * compare the two) */
        d->fused = !env_is("MP3D_PF_FUSED", "0");
    } else { /* staged copies: no buffer counts as mapped */
        (void)hipGetLastError();
        d->in.m = nullptr, d->out.m = nullptr, d->info.m = nullptr, d->done.m = nullptr;
    }
    if (d->ra_max && d->in.m) {
        const size_t K = (size_t)d->ra_max;
        /* the md region of a run (k_demux_fp stages no geometry): carry +
         * payloads of K maximal frames + the staging margin, zeroed */
        const size_t md_need = MP3D_RES_BYTES + K * MP3D_MAX_FRAME_BYTES + MP3D_MAX_FRAME_BYTES + 16 + 8192;
        /* zeroed on the handle's own stream and waited for (a null-stream
         * hipMemset does not order before kernels on non-blocking streams;
         * ADVICE r05) */
        if (d->b->md.grow(d->b, md_need) != MP3D_OK ||
            hipMemsetAsync(d->b->md, 0, d->b->md.cap, d->b->own) != hipSuccess ||
            hipStreamSynchronize(d->b->own) != hipSuccess)
            return fail(MP3D_E_NOMEM);
        /* frames, 64 zero bytes, then the frame offsets (4-B aligned) */
        const size_t in_bytes = K * MP3D_MAX_FRAME_BYTES + 64 + 4 + 4 * K;
        for (auto &u : d->run)
            if (u.in.alloc(in_bytes, hipHostMallocMapped, poison) != hipSuccess || u.in.map() != hipSuccess ||
                u.pcm.alloc(K * 2304 * sizeof(float), co, poison) != hipSuccess ||
                u.inf.alloc(K * sizeof(mp3d_frame_info), co, poison) != hipSuccess ||
                u.snap.grow(d->b, sizeof(StreamState)) != MP3D_OK || u.pcm.map() != hipSuccess ||
                u.inf.map() != hipSuccess || u.done.create(hipEventDisableTiming) != hipSuccess)
                return fail(MP3D_E_NOMEM);
    } else {
        d->ra_max = 0;
    }
    /* the helper thread that launches the next run, started here: started
     * on the first call that reads ahead past one run, its creation (tens of
     * us) landed on that call's latency */
    if (d->ra_max && d->ra_next_on && d->wk_on) {
        try {
            d->wk = std::thread(ra_worker, d);
        } catch (...) {
            d->wk_on = false; /* (the calling thread launches the next run) */
        }
    }
    *out = d;
    return MP3D_OK;
}

extern "C" int mp3d_dec_create(mp3d_dec **out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return mp3d_dec_create_on(dev, out);
}

extern "C" void mp3d_dec_destroy(mp3d_dec *d) {
    if (!d) return;
    dec_free(d);
}

static int ra_settle(mp3d_dec *d);
static int ra_join(mp3d_dec *d);

/* forget both read-ahead runs; a run still decoding is waited for first
 * (its host buffers are reused by the next fill) */
static void ra_drop(mp3d_dec *d) {
    for (auto &u : d->run) {
        if (u.pending) (void)hipEventSynchronize(u.done);
        u.pending = false;
        u.ents.clear();
    }
    d->ra_next = 0;
}

extern "C" void mp3d_dec_reset(mp3d_dec *d) {
    if (!d) return;
    (void)ra_join(d);
    ra_drop(d); /* the state is zeroed whole */
    d->ra_cool = d->ra_backoff = 0;
    d->broken = 0;
    (void)mp3d_batch_reset(d->b);
    d->frames = 0;
    d->kind = 0;
}

extern "C" int mp3d_dec_set_options(mp3d_dec *d, int flags) {
    if (!d) return MP3D_E_ARG;
    RCCHK(ra_settle(d)); /* frames read ahead under the old options */
    return mp3d_batch_set_options(d->b, flags);
}

extern "C" int mp3d_dec_stream_info(mp3d_dec *d, mp3d_stream_info *out) {
    if (!d || !out) return MP3D_E_ARG;
    RCCHK(ra_join(d));
    return mp3d_batch_stream_info(d->b, 1, out);
}

/* One frame through k_frame (one launch), then a poll of the mapped
 * completion word instead of a stream sync (~5 us less per
 * call).  The frame is in d->in[0, have).  Every few thousand polls a
 * stream query catches a kernel that faulted or aborted; a kernel that
 * never completes keeps the stream busy, so after ~1 ms of polling the host
 * stops spinning and blocks in hipStreamSynchronize (a hung kernel then
 * costs a blocked thread, not a spinning core). */
static int pf_fused(mp3d_dec *d, uint32_t have, bool f32, bool lsf) {
    mp3d_batch *b = d->b;
    hipStream_t s = b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const uint64_t off = 0;
    const uint32_t sz = MP3D_PF_BYTES;
    RCCHK(prepare_geometry(b, &off, &sz, 1, s)); /* uploaded once, then cached */
    RCCHK(flush_tail(b, s));                     /* k_frame reads the state from StreamState */
    mp3d_batch::Geo &g = b->geo[b->geo_i];
    const uint32_t seq = ++d->seq ? d->seq : ++d->seq; /* never 0, the word's initial value */
    RCCHK(stage_launch(b, nullptr, s, [&] {
        launch_frame(d->in.m, have, g.in_off(), g.in_len(), b->md, g.md_off(), b->st, b->rec, b->sideu, d->info.m,
                     b->opts, g_dev[b->device].tables, b->is_buf, b->meta, d->out.m, f32, lsf, d->done.m, seq, s);
    }));
    g.fresh = false; /* no event per call here: end_event covers it */
    for (uint32_t n = 1;; n++) {
        if (__atomic_load_n(d->done.p, __ATOMIC_ACQUIRE) == seq) return MP3D_OK;
        if ((n & 4095u) == 0) {
            const hipError_t e = n >= (64u << 12) ? hipStreamSynchronize(s) : hipStreamQuery(s);
            if (e == hipErrorNotReady) continue;
            HIPCHK(e);
            /* the stream is idle: the word must be there now */
            if (__atomic_load_n(d->done.p, __ATOMIC_ACQUIRE) == seq) return MP3D_OK;
            return MP3D_E_HIP;
        }
    }
}

/* Settle the read-ahead: the frames decoded ahead but not served are
 * dropped, and the device state is put back to "after the frames served":
 * the state saved before the run being served, then its frames served so
 * far decoded again (the same bytes, so the same state) -- or, when that
 * run was served whole and only the next one is ahead, the state saved
 * before the next run.  A no-op without a read-ahead. */
static int ra_settle_(mp3d_dec *d);
static int ra_settle(mp3d_dec *d) {
    if (d->broken) return d->broken;
    const int r = ra_settle_(d);
    if (r) d->broken = r; /* the restore may have run part-way */
    return r;
}
static int ra_settle_(mp3d_dec *d) {
    RCCHK(ra_join(d)); /* a launch still on the helper thread */
    mp3d_dec::Run &c = d->R(), &n = d->N();
    if (c.ents.empty() && n.ents.empty()) return MP3D_OK;
    const size_t served = d->ra_next;
    const bool cur_all = served == c.ents.size();
    if (cur_all && n.ents.empty()) { /* every frame was served: the state is where the caller is */
        ra_drop(d);
        d->ra_backoff = 0;
        return MP3D_OK;
    }
    d->ra_backoff = std::min(64, std::max(1, 2 * d->ra_backoff));
    d->ra_cool = d->ra_backoff;
    mp3d_batch *b = d->b;
    HIPCHK(hipSetDevice(b->device));
    RCCHK(own_after_last(b)); /* (the next run, if any, is on the own stream before this) */
    b->tail_live = -1; /* the tail holds the state after the last run */
    if (cur_all) {
        HIPCHK(hipMemcpyAsync(b->st, n.snap, sizeof(StreamState), hipMemcpyDeviceToDevice, b->own));
        HIPCHK(hipStreamSynchronize(b->own));
    } else {
        HIPCHK(hipMemcpyAsync(b->st, c.snap, sizeof(StreamState), hipMemcpyDeviceToDevice, b->own));
        if (served) {
            const uint32_t len = c.ents[served - 1].off + c.ents[served - 1].len;
            const FpRun fp = {c.in.m, len, (const uint32_t *)(c.in + c.fo_at), nullptr, c.snap};
            DecodeCall k;
            k.n = 1, k.F = (int)served, k.pcm = c.pcm.m, k.f32 = c.f32, k.infos = c.inf.m;
            k.mapped = true, k.seg_len = d->ra_seg, k.fp = &fp;
            RCCHK(batch_decode(b, k));
        } else {
            HIPCHK(hipStreamSynchronize(b->own));
        }
    }
    ra_drop(d);
    return MP3D_OK;
}

/* Stage run u from the call's buffer [buf, buf + bytes): the complete
 * frames found there (up to ra_max, located exactly as consecutive calls
 * would locate them: the first one with the stream-start rules when first is
 * set, the MPEG family locked to *kind once known) copied back to back into
 * u.in, then their offsets.  Host work only.  Returns the frames (0 for
 * fewer than 2: nothing staged); *o_out = their bytes, *kinds_out = their
 * families. */
static int ra_stage(mp3d_dec *d, mp3d_dec::Run &u, const uint8_t *buf, size_t bytes, bool first, int *kind,
                    uint32_t *o_out, int *kinds_out) {
    size_t cur = 0;
    uint32_t o = 0;
    int kinds = 0;
    u.ents.clear();
    for (int j = 0; j < d->ra_max; j++) {
        size_t pos = 0, have = 0;
        int fb = -1;
        if (pf_locate(buf + cur, bytes - cur, *kind, first && j == 0, false, &pos, &fb, &have) <= 0 ||
            have < (size_t)fb)
            break;
        memcpy(u.in + o, buf + cur + pos, (size_t)fb);
        u.ents.push_back({o, (uint32_t)fb, pos});
        const int k = host_frame_kind(buf + cur + pos);
        if (!*kind) *kind = k; /* checked again when each is served */
        kinds |= k;
        o += (uint32_t)fb;
        cur += pos + (size_t)fb;
    }
    if (u.ents.size() < 2) {
        u.ents.clear();
        return 0;
    }
    /* 64 zero bytes after the frames, then the frame offsets (k_demux_fp) */
    memset(u.in + o, 0, 64);
    u.fo_at = (o + 64 + 3) & ~3u;
    for (size_t j = 0; j < u.ents.size(); j++) ((uint32_t *)(u.in + u.fo_at))[j] = u.ents[j].off;
    *o_out = o;
    *kinds_out = kinds;
    return (int)u.ents.size();
}

/* Decode a staged run in one batch call -- synchronously, or launched
 * without waiting (async: the next run; its done event is recorded). */
static int ra_launch(mp3d_dec *d, mp3d_dec::Run &u, uint32_t o, int kinds, bool f32, bool async) {
    mp3d_batch *b = d->b;
    HIPCHK(hipSetDevice(b->device));
    RCCHK(own_after_last(b));
    /* the previous run's synthesis tail is flushed into the state, and the
     * state before this run saved to u.snap (for ra_settle), by k_demux_fp */
    const float *tail = b->tail_live >= 0 ? b->st_tail[b->tail_live].p : nullptr;
    b->tail_live = -1;
    const FpRun fp = {u.in.m, o, (const uint32_t *)(u.in + u.fo_at), tail, u.snap};
    DecodeCall k;
    k.n = 1, k.F = (int)u.ents.size(), k.pcm = u.pcm.m, k.f32 = f32, k.infos = u.inf.m;
    k.kinds = kinds, k.mapped = true, k.seg_len = d->ra_seg, k.fp = &fp, k.async = async;
    RCCHK(batch_decode(b, k));
    if (async && d->dbg_fail && ++d->dbg_launches == d->dbg_fail) {
        (void)hipStreamSynchronize(b->own);
        return MP3D_E_HIP;
    }
    u.f32 = f32;
    u.pending = async;
    if (async) HIPCHK(hipEventRecord(u.done, b->own));
    return MP3D_OK;
}

/* wait for the helper thread's launch, if one was handed over; its status */
static int ra_join(mp3d_dec *d) {
    if (!d->wk.joinable()) return MP3D_OK;
    std::unique_lock<std::mutex> lk(d->wk_mu);
    d->wk_cv.wait(lk, [d] { return !d->wk_job; });
    const int rc = d->wk_rc;
    d->wk_rc = 0;
    return rc;
}

static void ra_worker(mp3d_dec *d) {
    for (;;) {
        std::unique_lock<std::mutex> lk(d->wk_mu);
        d->wk_cv.wait(lk, [d] { return d->wk_job || d->wk_quit; });
        if (!d->wk_job) return; /* quit */
        const mp3d_dec::WkJob j = d->wk_arg;
        lk.unlock();
        if (d->wk_delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(d->wk_delay_us));
        const int rc = ra_launch(d, *j.u, j.o, j.kinds, j.f32, true);
        lk.lock();
        if (rc) {
            j.u->ents.clear(); /* (the caller sees no next run, and rc at its next join) */
            d->broken = rc;    /* the state may be past the served frames */
        }
        d->wk_rc = rc;
        d->wk_job = false;
        lk.unlock();
        d->wk_cv.notify_all();
    }
}

/* Fill run u synchronously: stage + launch + wait.  Returns 1 for a run of
 * >= 2 frames, else 0 and nothing launched. */
static int ra_fill(mp3d_dec *d, mp3d_dec::Run &u, const uint8_t *buf, size_t bytes, bool f32, bool first, int *kind) {
    uint32_t o = 0;
    int kinds = 0;
    if (!ra_stage(d, u, buf, bytes, first, kind, &o, &kinds)) return 0;
    const int r = ra_launch(d, u, o, kinds, f32, false);
    if (r) {
        u.ents.clear();
        d->broken = r;
        return r;
    }
    return 1;
}

/* the next run: the frames after run[cur] in the call's buffer (which starts
 * at run[cur]'s first frame), staged here and launched by the helper thread,
 * decoding behind the calls served from run[cur] */
static int ra_launch_next(mp3d_dec *d, const uint8_t *buf, size_t bytes, bool f32) {
    if (!d->ra_next_on) return MP3D_OK;
    size_t at = 0;
    for (const auto &e : d->R().ents) at += e.pos + e.len;
    if (at >= bytes) return MP3D_OK;
    /* the family lock: the stream's, or its first frame's (run[cur]'s first) */
    int kind = d->kind ? d->kind : host_frame_kind(buf + d->R().ents[0].pos);
    mp3d_dec::Run &u = d->N();
    uint32_t o = 0;
    int kinds = 0;
    if (!ra_stage(d, u, buf + at, bytes - at, false, &kind, &o, &kinds)) return MP3D_OK;
    if (!d->wk_on) {
        const int r = ra_launch(d, u, o, kinds, f32, true);
        if (r) {
            u.ents.clear();
            d->broken = r;
        }
        return r;
    }
    if (!d->wk.joinable()) d->wk = std::thread(ra_worker, d);
    {
        std::lock_guard<std::mutex> lk(d->wk_mu);
        d->wk_arg = {&u, o, kinds, f32};
        d->wk_job = true;
    }
    d->wk_cv.notify_all();
    return MP3D_OK;
}

static int decode_frame(mp3d_dec *d, const uint8_t *buf, size_t bytes, void *pcm, bool f32, bool last,
                        mp3d_frame_info *info) {
    if (!d || !buf) return MP3D_E_ARG;
    if (d->broken) return d->broken;
    mp3d_frame_info tmp;
    if (!info) info = &tmp;
    memset(info, 0, sizeof(*info));
    size_t pos = 0, have = 0;
    int fb = -1;
    /* next frame (ID3v2 / junk skipped); a final frame cut short only with
     * MP3D_FRAME_LAST: decoded with the missing bytes as zeros (k_demux) */
    const int loc = pf_locate(buf, bytes, d->kind, d->frames == 0, last, &pos, &fb, &have);
    /* a frame read ahead: the same bytes at the same place, the same sink */
    auto same = [&](const mp3d_dec::Run &u, const mp3d_dec::RaEnt &e) {
        return loc > 0 && f32 == u.f32 && pos == e.pos && have == (size_t)fb && (size_t)fb == e.len &&
               !memcmp(buf + pos, u.in + e.off, e.len);
    };
    if (d->ra_next < d->R().ents.size()) {
        if (!same(d->R(), d->R().ents[d->ra_next])) RCCHK(ra_settle(d));
    } else if (!d->R().ents.empty()) {
        /* the run being served is used up: on to the next run when this call
         * asks for its first frame (it was decoding behind the served calls),
         * and launch the one after it */
        RCCHK(ra_join(d)); /* the helper's launch of it (its status) */
        mp3d_dec::Run &n = d->N();
        if (!n.ents.empty() && same(n, n.ents[0])) {
            if (n.pending) HIPCHK(hipEventSynchronize(n.done));
            n.pending = false;
            d->R().ents.clear();
            d->cur ^= 1;
            d->ra_next = 0;
            d->ra_backoff = 0;
            RCCHK(ra_launch_next(d, buf, bytes, f32));
        } else {
            RCCHK(ra_settle(d)); /* (served whole: a no-op unless a next run is dropped) */
        }
    }
    if (loc <= 0) {
        info->frame_bytes = (int)pos;
        return loc;
    }
    bool cached = d->ra_next < d->R().ents.size();
    if (!cached) RCCHK(ra_join(d)); /* the batch handle is used below */
    if (!cached && have == (size_t)fb && d->ra_max) {
        if (d->ra_cool > 0) { /* backing off after a wasted read-ahead */
            d->ra_cool--;
        } else {
            int kind = d->kind;
            const int r = ra_fill(d, d->R(), buf, bytes, f32, d->frames == 0, &kind);
            if (r < 0) return r;
            cached = r == 1;
            if (cached) {
                d->ra_next = 0;
                RCCHK(ra_launch_next(d, buf, bytes, f32));
            }
        }
    }
    mp3d_frame_info fi;
    const void *out;
    if (cached) {
        const mp3d_dec::Run &c = d->R();
        fi = c.inf[d->ra_next];
        out = (const uint8_t *)c.pcm + d->ra_next * 2304 * (f32 ? sizeof(float) : sizeof(int16_t));
        d->ra_next++;
    } else {
        const uint64_t off = 0;
        const uint32_t sz = MP3D_PF_BYTES;
        memcpy(d->in, buf + pos, have); /* have <= fb <= MP3D_MAX_FRAME_BYTES */
        const int kind = host_frame_kind(buf + pos); /* 1 MPEG-1, 2 LSF */
        if (d->fused) {
            RCCHK(pf_fused(d, (uint32_t)have, f32, kind == 2));
        } else {
            memset(d->in + have, 0, MP3D_PF_BYTES - have);
            /* mapped pinned buffers: the kernels read the frame and write PCM +
             * info in place (three launches + one sync); else staged copies
             * of the whole row (only its audio is read below) */
            const bool mapped = d->in.m != nullptr;
            DecodeCall k;
            k.frames = mapped ? d->in.m : d->in.p, k.offsets = &off, k.sizes = &sz, k.n = 1, k.F = 1;
            k.pcm = mapped ? d->out.m : d->out.p, k.f32 = f32, k.infos = mapped ? d->info.m : d->info.p;
            k.clobber_unwritten = true, k.kinds = kind, k.mapped = mapped;
            RCCHK(batch_decode(d->b, k));
        }
        fi = *d->info.p;
        out = d->out.p;
    }
    d->frames++;
    if (fi.frame_bytes) d->kind = host_frame_kind(buf + pos);
    *info = fi;
    info->frame_bytes = (int)pos + (int)std::min<size_t>((size_t)fi.frame_bytes, have);
    if (fi.samples && pcm) memcpy(pcm, out, (f32 ? sizeof(float) : sizeof(int16_t)) * (size_t)fi.samples * fi.channels);
    return fi.samples;
}

extern "C" int mp3d_decode_frame(mp3d_dec *d, const uint8_t *buf, size_t bytes, int16_t *pcm, mp3d_frame_info *info) {
    return decode_frame(d, buf, bytes, pcm, false, false, info);
}

extern "C" int mp3d_decode_frame_f32(mp3d_dec *d, const uint8_t *buf, size_t bytes, float *pcm,
                                     mp3d_frame_info *info) {
    return decode_frame(d, buf, bytes, pcm, true, false, info);
}

extern "C" int mp3d_decode_frame_ex(mp3d_dec *d, const uint8_t *buf, size_t bytes, void *pcm, int flags,
                                    mp3d_frame_info *info) {
    if (flags & ~(MP3D_FRAME_F32 | MP3D_FRAME_LAST)) return MP3D_E_ARG;
    return decode_frame(d, buf, bytes, pcm, (flags & MP3D_FRAME_F32) != 0, (flags & MP3D_FRAME_LAST) != 0, info);
}

extern "C" int mp3d_dec_get_state(mp3d_dec *d, void *buf) {
    if (!d) return MP3D_E_ARG;
    RCCHK(ra_settle(d)); /* the state after the frames served, not after those read ahead */
    return mp3d_batch_get_state(d->b, 0, 1, buf);
}

extern "C" int mp3d_dec_set_state(mp3d_dec *d, const void *buf) {
    if (!d || !buf) return MP3D_E_ARG;
    /* a refused blob writes nothing (mp3d.h): checked BEFORE the read-ahead
     * is forgotten, so the decoder stays at the frame it served */
    (void)ra_join(d); /* (a failed launch left d->broken, which a new state clears) */
    RCCHK(blob_check(d->b, 1, buf));
    ra_drop(d); /* replaced whole: nothing read ahead applies */
    RCCHK(mp3d_batch_set_state(d->b, 0, 1, buf));
    d->broken = 0; /* a whole new state: a failed read-ahead no longer matters */
    /* host mirror of the family lock and "past the stream start" (ID3v2 skip) */
    StreamState h;
    HIPCHK(hipMemcpy(&h, d->b->st, sizeof(h), hipMemcpyDeviceToHost));
    d->kind = h.kind;
    d->frames = (long)h.frames + (h.tag_info ? 1 : 0);
    return MP3D_OK;
}
