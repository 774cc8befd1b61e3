/*
 * mp3d_batch.cpp -- the batch handle of the C ABI (include/mp3d.h): create
 * and destroy, stream geometry, the three-kernel decode and its taps, stream
 * info and per-stream state save / restore.
 *
 * No CPU decode path exists here: every frame is decoded by the HIP kernels
 * in mp3d_demux.hip, mp3d_huffman.hip and mp3d_synth.hip; without a device
 * the create calls fail.
 */
#include "mp3d_host.h"

using namespace mp3d;

hipError_t mp3d::state_clear(StreamState *st, int n, hipStream_t s) {
    hipError_t e = hipMemsetAsync(st, 0, sizeof(StreamState) * (size_t)n, s);
    if (e == hipSuccess)
        e = hipMemset2DAsync(&st[0].fmt, sizeof(StreamState), MP3D_STATE_FMT_BYTE, sizeof(uint32_t), (size_t)n, s);
    return e;
}

static bool poison_env() { return env_flag("MP3D_DEBUG_POISON"); }

/* Frames per k_synth segment for n streams x F frames: few streams leave
 * the chip idle (one wave walks one stream), so each stream is split into
 * frame-parallel segments (one wave each, warm-up frames before; k_synth)
 * until one round of resident waves (4 per SIMD) is in the grid, keeping
 * segments >= min_len frames (C2, 1 024 x 64: 4 segments of 16 frames;
 * at 3 waves per SIMD, 2 rounds of 11 frames measured 4 % slower than one
 * of 22, tools/dbg/job_c2_seg.sh).
 * MP3D_SEG_FRAMES overrides (0 = never split). */
static int seg_frames(int n, int F, int n_cu, int min_len) {
    int seg_len = F;
    const long long want = 4LL * 4 * n_cu; /* one round at 4 waves per SIMD */
    if ((long long)n < want && F >= 2 * min_len) {
        const int nseg = (int)std::min<long long>((want + n - 1) / n, F / min_len);
        seg_len = (F + nseg - 1) / nseg;
    }
    const int v = env_int("MP3D_SEG_FRAMES", -1, -1, F);
    if (v > 0 || (v == 0 && env_is("MP3D_SEG_FRAMES", "0"))) seg_len = v ? v : F;
    return seg_len;
}

/* where k_synth takes each stream's overlap + fifo from and puts them:
 * in = the live tail when it holds these n streams (else StreamState, after
 * copying back a tail of another shape); out = the other tail when the
 * call is segmented (the first segment may still be reading the state),
 * else StreamState.  tail_commit() after the launch. */
struct TailPlan {
    const float *in = nullptr;
    float *out = nullptr;
    int t_out = 0;
};
static void tail_commit(mp3d_batch *b, int n, int F, int seg_len, const TailPlan &tp) {
    if (seg_len < F) {
        b->tail_live = tp.t_out;
        b->tail_n = n;
    }
}

static constexpr size_t STATE_TAIL = sizeof(((StreamState *)0)->overlap) + sizeof(((StreamState *)0)->fifo);

int mp3d::flush_tail(mp3d_batch *b, hipStream_t s) {
    if (b->tail_live < 0) return MP3D_OK;
    HIPCHK(hipMemcpy2DAsync(&b->st[0].overlap[0][0][0], sizeof(StreamState), b->st_tail[b->tail_live], STATE_TAIL,
                            STATE_TAIL, b->tail_n, hipMemcpyDeviceToDevice, s));
    b->tail_live = -1;
    return MP3D_OK;
}

static int tail_plan(mp3d_batch *b, int n, int F, int seg_len, hipStream_t s, TailPlan *tp) {
    if (b->tail_live >= 0 && (seg_len >= F || b->tail_n != n)) RCCHK(flush_tail(b, s));
    tp->in = b->tail_live >= 0 ? b->st_tail[b->tail_live].p : nullptr;
    tp->t_out = b->tail_live >= 0 ? b->tail_live ^ 1 : 0;
    tp->out = nullptr;
    if (seg_len < F) {
        DevBuf<float> &t = b->st_tail[tp->t_out];
        const size_t need = STATE_TAIL * (size_t)n;
        const bool fresh = need > t.cap;
        RCCHK(t.grow(b, need));
        /* k_synth writes the fifo slots the synthesis reads back (slot 0 only
         * at the columns some lane's window needs): zero the rest once, as
         * StreamState is, so a flushed tail leaves the same state bytes */
        if (fresh) HIPCHK(hipMemsetAsync(t, 0, t.cap, s));
        tp->out = t;
    }
    return MP3D_OK;
}

PtrKind mp3d::ptr_kind(const void *p, int device) {
    if (!p) return PTR_HOST;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return PTR_HOST;
    }
    if (a.type == hipMemoryTypeManaged) return PTR_DEV;
    if (a.type != hipMemoryTypeDevice) return PTR_HOST;
    return a.device == device ? PTR_DEV : PTR_OTHER_DEV;
}

extern "C" int mp3d_batch_create(int device, int max_streams, int max_frames, mp3d_batch **out) {
    if (!out || max_streams <= 0 || max_frames <= 0) return MP3D_E_ARG;
    *out = nullptr;
    RCCHK(device_init(device));
    mp3d_batch *b = new (std::nothrow) mp3d_batch;
    if (!b) return MP3D_E_NOMEM;
    b->device = device;
    b->max_streams = max_streams;
    b->max_frames = max_frames;
    b->poison = poison_env();
    /* the streams before the buffers: a poisoned allocation is filled on the own stream */
    const size_t ns = (size_t)max_streams, fr = ns * max_frames, units = fr * 4;
    bool ok = hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&b->copy, hipStreamNonBlocking) == hipSuccess &&
              b->ev_done.create(hipEventDisableTiming) == hipSuccess;
    for (auto &g : b->geo)
        ok = ok && g.h.alloc(20 * ns, hipHostMallocDefault, b->poison) == hipSuccess &&
             g.staged.create(hipEventDisableTiming) == hipSuccess &&
             g.freed.create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        mp3d_batch_destroy(b);
        return MP3D_E_HIP;
    }
    int r = b->st_mem.grow(b, sizeof(StreamState) * ns);
    if (!r) r = b->rec.grow(b, sizeof(FrameRec) * fr);
    if (!r) r = b->sideu.grow(b, sizeof(uint64_t) * units);
    if (!r) r = b->is_buf.grow(b, sizeof(int16_t) * MP3D_IS_ROW * units);
    if (!r) r = b->meta.grow(b, sizeof(UnitMeta) * units);
    if (!r) r = b->rank.grow(b, sizeof(uint32_t) * units);
    for (auto &g : b->geo)
        if (!r) r = g.d.grow(b, 20 * ns);
    if (!r) r = b->d_infos.grow(b, sizeof(mp3d_frame_info) * fr);
    if (!r) r = b->d_work.grow(b, 256);
    if (r) {
        mp3d_batch_destroy(b);
        return r;
    }
    b->st = b->st_mem;
    if (env_set("MP3D_DEBUG_ADDR")) /* placement diagnostics (tools/dbg/place.py) */
        fprintf(stderr, "mp3d: st %p rec %p sideu %p is_buf %p meta %p infos %p\n", (void *)b->st, (void *)b->rec,
                (void *)b->sideu, (void *)b->is_buf, (void *)b->meta, (void *)b->d_infos);
    /* zeroed on the handle's own stream and waited for: a null-stream
     * hipMemset is asynchronous for device memory and does not order before
     * kernels on non-blocking streams (a first call could read the previous
     * owner's bytes as its streams' state) */
    if (state_clear(b->st, max_streams, b->own) != hipSuccess ||
        hipMemsetAsync(b->d_work, 0, 256, b->own) != hipSuccess || hipStreamSynchronize(b->own) != hipSuccess) {
        mp3d_batch_destroy(b);
        return MP3D_E_HIP;
    }
    *out = b;
    return MP3D_OK;
}

extern "C" void mp3d_batch_destroy(mp3d_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->ev_done) (void)hipEventSynchronize(b->ev_done);
    if (b->own) (void)hipStreamSynchronize(b->own);
    if (b->copy) (void)hipStreamSynchronize(b->copy);
    if (b->own) (void)hipStreamDestroy(b->own);
    if (b->copy) (void)hipStreamDestroy(b->copy);
    delete b; /* frees every device and pinned buffer and every event, after the waits above */
}

extern "C" int mp3d_batch_reset(mp3d_batch *b) {
    if (!b) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    RCCHK(own_after_last(b));
    b->tail_live = -1; /* the state is zeroed whole */
    HIPCHK(state_clear(b->st, b->max_streams, b->own));
    if (b->rs.st) HIPCHK(hipMemsetAsync(b->rs.st, 0, sizeof(RsState) * (size_t)b->max_streams, b->own));
    RCCHK(stages_restart(b, 0, b->max_streams, b->own));
    HIPCHK(hipStreamSynchronize(b->own));
    return MP3D_OK;
}

extern "C" int mp3d_batch_set_options(mp3d_batch *b, int flags) {
    if (!b || (flags & ~MP3D_OPT_CRC_CHECK)) return MP3D_E_ARG;
    b->opts = flags;
    return MP3D_OK;
}

/* waits for this handle's work only: its last call (through ev_done, on
 * whatever stream it ran) and its own stream, never the whole device */
extern "C" int mp3d_batch_sync(mp3d_batch *b) {
    if (!b) return MP3D_E_ARG;
    HIPCHK(hipSetDevice(b->device));
    if (b->last_s && b->last_s != b->own) HIPCHK(hipEventSynchronize(b->ev_done));
    HIPCHK(hipStreamSynchronize(b->own));
    return MP3D_OK;
}

extern "C" int mp3d_batch_set_timing(mp3d_batch *b, int enable) {
    if (!b) return MP3D_E_ARG;
    b->timing = enable != 0;
    return MP3D_OK;
}

extern "C" int mp3d_batch_kernel_times(mp3d_batch *b, float *us3) {
    if (!b || !us3) return MP3D_E_ARG;
    if (!b->timing) return MP3D_E_ARG;
    HIPCHK(hipEventSynchronize(b->ev[3]));
    for (int i = 0; i < 3; i++) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, b->ev[i], b->ev[i + 1]));
        us3[i] = ms * 1000.f;
    }
    return MP3D_OK;
}

/* batches from this many streams take k_walk + k_mdcopy */
#define MP3D_WIDE_STREAMS 256
/* MP3D_DEMUX=lane | wave forces the demux path (tests run both) */
static bool demux_wide(int n) {
    return env_is("MP3D_DEMUX", "lane") || (n >= MP3D_WIDE_STREAMS && !env_is("MP3D_DEMUX", "wave"));
}

/* MP3D_SYNTH_LONGPATH=0 sends every granule through k_synth's general phase
 * Q and alias step (tests compare the two paths bit for bit); default on */
static bool synth_longpath() { return !env_is("MP3D_SYNTH_LONGPATH", "0"); }

/* batches of at most this many units (frame granule channels) decode one
 * unit per wave (k_huffman_wave); MP3D_HUFF=wave | lane forces the kernel */
#define MP3D_WAVE_HUFF_UNITS 1024
static bool huffman_wave(int n_units) {
    return env_is("MP3D_HUFF", "wave") || (n_units <= MP3D_WAVE_HUFF_UNITS && !env_is("MP3D_HUFF", "lane"));
}

/* a call compares the new geometry with the current slot's and skips the
 * copy when it is unchanged (host time: a memcmp of up to 0.8 MB while the
 * GPU runs the previous call; the staging copy it saves ran on the GPU's
 * timeline between calls, 29 us of copy + 17 us before the next kernel at
 * 65 536 streams, memory-copy trace, round 5) */
#define MP3D_GEO_CACHE_STREAMS (1 << 30)

/* Stage the call's stream geometry (input offsets and sizes, md-region
 * offsets) into the next device slot, asynchronously (struct Geo), size the
 * md region, and make stream s wait for the copy.  Never blocks the host
 * except on the copy of two calls ago. */
int mp3d::prepare_geometry(mp3d_batch *b, const uint64_t *offsets, const uint32_t *sizes, int n, hipStream_t s) {
    {
        mp3d_batch::Geo &g = b->geo[b->geo_i];
        if (n <= MP3D_GEO_CACHE_STREAMS && g.n == n && !memcmp(g.h, offsets, sizeof(uint64_t) * n) &&
            !memcmp(g.h + 2 * (size_t)n, sizes, sizeof(uint32_t) * n)) {
            HIPCHK(hipStreamWaitEvent(s, g.staged, 0)); /* a no-op once the copy is done */
            return MP3D_OK;
        }
    }
    b->geo_i ^= 1;
    mp3d_batch::Geo &g = b->geo[b->geo_i];
    /* the slot holds no valid geometry until its copy is queued: a failed
     * stage below can never be served from the cache by a retried call */
    g.n = -1;
    HIPCHK(hipEventSynchronize(g.staged)); /* this slot's last copy has read g.h */
    uint64_t *h_md = g.h + n;
    size_t o = 0;
    for (int i = 0; i < n; i++) {
        h_md[i] = o;
        /* carry-in + payloads; a cut-short final frame is completed with
         * zeros, so allow one maximal frame beyond the stream's bytes */
        o += ((size_t)sizes[i] + MP3D_RES_BYTES + MP3D_MAX_FRAME_BYTES + 16 + 15) & ~(size_t)15;
    }
    memcpy(g.h, offsets, sizeof(uint64_t) * n);
    memcpy(g.h + 2 * (size_t)n, sizes, sizeof(uint32_t) * n);
    /* growing md frees the old region: hipFree waits for the device */
    const size_t md_was = b->md.cap;
    RCCHK(b->md.grow(b, o + 8192));
    /* a new region starts zeroed: the Huffman staging reads whole words up
     * to 2 past a unit's end, and a corrupt unit may decode past its
     * payload -- those bits then read as zeros (FFmpeg's buffer padding),
     * never as a previous allocation's bytes */
    if (b->md.cap != md_was) HIPCHK(hipMemsetAsync(b->md, 0, b->md.cap, s));
    /* after the call that last read this slot */
    HIPCHK(hipStreamWaitEvent(b->copy, g.fresh ? g.freed : end_event(b), 0));
    HIPCHK(hipMemcpyAsync(g.d, g.h, 20 * (size_t)n, hipMemcpyHostToDevice, b->copy));
    HIPCHK(hipEventRecord(g.staged, b->copy));
    HIPCHK(hipStreamWaitEvent(s, g.staged, 0));
    g.n = n;
    return MP3D_OK;
}

/* The front half's kernels on stream s between events 0 and 2 of the timing
 * chain: `demux` (the caller's launch of k_demux / k_walk or k_demux_fp, for
 * call_seq as counted here), then k_huffman over the md region it filled,
 * the streams' offsets in it at md_off.  wide: the demux is k_walk. */
template <class D>
static int front_kernels(mp3d_batch *b, bool wide, D &&demux, const uint64_t *md_off, int n, int F, bool huff_wave,
                         uint32_t *rank, hipStream_t s) {
    DeviceCtx &dc = g_dev[b->device];
    RCCHK(core_mark(b, 0, s));
    if (++b->call_seq == 0) b->call_seq = 1; /* (d_work[1] starts at 0) */
    b->fam_ok = wide;
    RCCHK(core_launch(b, 1, s, demux));
    return core_launch(b, 2, s, [&] {
        launch_huffman(b->md, md_off, b->rec, b->sideu, dc.tables, b->is_buf, b->meta, n, F, dc.n_cu, huff_wave,
                       b->d_work, rank, s);
    });
}

/* Front half shared by decode and huffman_only: input staging, k_demux,
 * k_huffman; the frame infos go to dinf (device-accessible).  c.mapped: the
 * frames need no staging copy. */
static int run_front(mp3d_batch *b, const DecodeCall &c, mp3d_frame_info *dinf, hipStream_t s, bool *sync_needed) {
    const int n = c.n, F = c.F;
    if (!c.frames || !c.offsets || !c.sizes || n <= 0 || F <= 0) return MP3D_E_ARG;
    if (n > b->max_streams || F > b->max_frames) return MP3D_E_CAPACITY;
    RCCHK(call_begin(b, s)); /* (the demux and Huffman stages never touch a live tail's overlap / fifo) */
    uint64_t total = 0;
    for (int i = 0; i < n; i++) total = std::max<uint64_t>(total, c.offsets[i] + c.sizes[i]);
    const uint8_t *din = c.frames;
    if (!c.mapped && !is_device_ptr(c.frames, b->device)) {
        RCCHK(b->d_in.grow(b, total + 64));
        HIPCHK(hipMemcpyAsync(b->d_in, c.frames, total, hipMemcpyDefault, s));
        din = b->d_in;
        *sync_needed = true;
    }
    RCCHK(prepare_geometry(b, c.offsets, c.sizes, n, s));
    mp3d_batch::Geo &g = b->geo[b->geo_i];
    /* demux + main-data gather: lane-per-stream walk + payload copy for wide
     * batches, one wave per stream below MP3D_WIDE_STREAMS (fewer launches) */
    const bool wide = demux_wide(n);
    RCCHK(front_kernels(
        b, wide,
        [&] {
            launch_demux(din, g.in_off(), g.in_len(), b->md, g.md_off(), b->st, b->rec, b->sideu, dinf, n, F, b->opts,
                         wide, b->d_work + 1, b->call_seq, s);
        },
        g.md_off(), n, F, huffman_wave(n * F * 4), b->rank, s));
    HIPCHK(hipEventRecord(g.freed, s)); /* the slot's last reader */
    g.fresh = true;
    return MP3D_OK;
}

/* the front half for one run of pre-located frames (FpRun, mp3d_host.h) */
static int run_front_fp(mp3d_batch *b, const FpRun &fp, int F, mp3d_frame_info *dinf, hipStream_t s) {
    if (b->max_streams != 1 || F <= 0 || F > 64 || F > b->max_frames) return MP3D_E_ARG;
    RCCHK(call_begin(b, s));
    if (b->md.cap < (size_t)fp.len + MP3D_RES_BYTES + 8192) return MP3D_E_CAPACITY; /* sized at create */
    /* md offset of the one stream: a zero word of d_work (d_work[4..5]) */
    return front_kernels(
        b, false,
        [&] {
            launch_demux_fp(fp.in, fp.len, fp.fo, b->md, b->st, fp.tail_in, fp.snap, b->rec, b->sideu, dinf, F,
                            b->opts, s);
        },
        (const uint64_t *)(b->d_work + 4), 1, F, true, nullptr, s);
}

int mp3d::batch_decode(mp3d_batch *b, const DecodeCall &c) {
    if (!b || !c.pcm || (c.async && !c.mapped)) return MP3D_E_ARG;
    const int n = c.n, F = c.F;
    void *const pcm = c.pcm;
    mp3d_frame_info *const infos = c.infos;
    const bool f32 = c.f32, mapped = c.mapped;
    hipStream_t s = c.hip_stream ? (hipStream_t)c.hip_stream : b->own;
    CallEnd done{b, s};
    bool sync_needed = mapped;
    /* frame infos: written in place when the caller's array is device memory
     * (or the per-frame decoder's mapped buffer), else into d_infos and
     * copied to the host after the call */
    const bool inf_host = infos && !mapped && !is_device_ptr(infos, b->device); /* or another GPU's */
    mp3d_frame_info *dinf = infos && !inf_host ? infos : b->d_infos.p;
    RCCHK(c.fp ? run_front_fp(b, *c.fp, F, dinf, s) : run_front(b, c, dinf, s, &sync_needed));
    const size_t PB = f32 ? sizeof(float) : sizeof(int16_t), row = 2304 * PB;
    const size_t pcm_bytes = (size_t)n * F * row;
    void *dpcm = pcm;
    const PtrKind pk = mapped ? PTR_DEV : ptr_kind(pcm, b->device);
    bool pcm_host = pk == PTR_HOST;
    if (pk != PTR_DEV) {
        RCCHK(b->d_pcm.grow(b, pcm_bytes));
        dpcm = b->d_pcm;
        /* another GPU's buffer: its rows the kernel does not write keep their
         * bytes, as in place (copied over, decoded into, copied back) */
        if (pk == PTR_OTHER_DEV) HIPCHK(hipMemcpyAsync(dpcm, pcm, pcm_bytes, hipMemcpyDefault, s));
    }
    DeviceCtx &dc = g_dev[b->device];
    /* few streams: frame-parallel segments per stream (>= 4 frames each,
     * or the caller's seg_len) */
    const int seg_len = c.seg_len > 0 ? std::min(F, c.seg_len) : seg_frames(n, F, dc.n_cu, 4);
    TailPlan tp;
    RCCHK(tail_plan(b, n, F, seg_len, s, &tp));
    RCCHK(core_launch(b, 3, s, [&] {
        launch_synth(b->rec, b->is_buf, b->meta, dc.tables, b->st, dpcm, f32, n, F, c.kinds, seg_len, tp.out, tp.in,
                     b->fam_ok ? b->d_work + 1 : nullptr, b->call_seq, dc.n_cu, synth_longpath(), s);
    }));
    tail_commit(b, n, F, seg_len, tp);
    const size_t ib = sizeof(mp3d_frame_info) * (size_t)n * F;
    if (pcm_host && !c.clobber_unwritten) {
        /* A host sink is read back whole, but each row keeps the caller's
         * bytes the kernel did not write (rows without audio, the second
         * half of a mono / LSF row): those few spans are saved from the
         * caller's buffer and put back after the copy -- no host-to-device
         * copy of the whole PCM buffer first. */
        std::vector<mp3d_frame_info> tmp;
        mp3d_frame_info *hi = inf_host ? infos : nullptr;
        if (!hi) {
            tmp.resize((size_t)n * F);
            hi = tmp.data();
        }
        HIPCHK(hipMemcpyAsync(hi, dinf, ib, hipMemcpyDefault, s));
        HIPCHK(hipStreamSynchronize(s));
        std::vector<size_t> at;
        std::vector<uint8_t> kept;
        for (size_t i = 0; i < (size_t)n * F; i++) {
            const size_t w = (size_t)hi[i].samples * (size_t)hi[i].channels * PB;
            if (w >= row) continue;
            at.push_back(i);
            kept.insert(kept.end(), (const uint8_t *)pcm + i * row + w, (const uint8_t *)pcm + (i + 1) * row);
        }
        HIPCHK(hipMemcpyAsync(pcm, dpcm, pcm_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        size_t k = 0;
        for (size_t i : at) {
            const size_t w = (size_t)hi[i].samples * (size_t)hi[i].channels * PB;
            memcpy((uint8_t *)pcm + i * row + w, kept.data() + k, row - w);
            k += row - w;
        }
        return MP3D_OK;
    }
    if (pk != PTR_DEV) { /* another GPU's buffer, or internal callers that read only the rows with audio */
        HIPCHK(hipMemcpyAsync(pcm, dpcm, pcm_bytes, hipMemcpyDefault, s));
        sync_needed = pcm_host;
    }
    if (inf_host) {
        HIPCHK(hipMemcpyAsync(infos, b->d_infos, ib, hipMemcpyDefault, s));
        sync_needed = sync_needed || ptr_kind(infos, b->device) == PTR_HOST;
    }
    if (sync_needed && !c.async) HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

/* the public decodes: the call as the ABI states it, the options at their defaults */
static int decode_public(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets, const uint32_t *sizes, int n,
                         int F, void *pcm, bool f32, mp3d_frame_info *infos, void *hip_stream) {
    DecodeCall c;
    c.frames = frames, c.offsets = offsets, c.sizes = sizes, c.n = n, c.F = F;
    c.pcm = pcm, c.f32 = f32, c.infos = infos, c.hip_stream = hip_stream;
    return batch_decode(b, c);
}

extern "C" int mp3d_batch_decode(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets, const uint32_t *sizes,
                                 int n, int F, int16_t *pcm, mp3d_frame_info *infos, void *hip_stream) {
    return decode_public(b, frames, offsets, sizes, n, F, pcm, false, infos, hip_stream);
}

extern "C" int mp3d_batch_decode_f32(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                     const uint32_t *sizes, int n, int F, float *pcm, mp3d_frame_info *infos,
                                     void *hip_stream) {
    return decode_public(b, frames, offsets, sizes, n, F, pcm, true, infos, hip_stream);
}

extern "C" int mp3d_batch_huffman_only(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                       const uint32_t *sizes, int n, int F, int16_t *is_out, uint8_t *sf_out,
                                       void *hip_stream) {
    if (!b) return MP3D_E_ARG;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    CallEnd done{b, s};
    bool sync_needed = false;
    size_t units = (size_t)n * F * 4;
    if (n > 0 && F > 0 && n <= b->max_streams && F <= b->max_frames) {
        /* k_huffman stores only each row's nonzero prefix (nz_end); the tap
         * returns whole rows, so clear them first */
        RCCHK(call_begin(b, s));
        HIPCHK(hipMemsetAsync(b->is_buf, 0, units * MP3D_IS_ROW * sizeof(int16_t), s));
    }
    DecodeCall c; /* (its input only: the tap has no sink) */
    c.frames = frames, c.offsets = offsets, c.sizes = sizes, c.n = n, c.F = F;
    RCCHK(run_front(b, c, b->d_infos, s, &sync_needed));
    if (is_out) {
        HIPCHK(hipMemcpy2DAsync(is_out, 576 * sizeof(int16_t), b->is_buf, MP3D_IS_ROW * sizeof(int16_t),
                                576 * sizeof(int16_t), units, hipMemcpyDefault, s));
        sync_needed |= ptr_kind(is_out, b->device) == PTR_HOST;
    }
    if (sf_out) {
        HIPCHK(hipMemcpy2DAsync(sf_out, 40, b->meta, sizeof(UnitMeta), 40, units, hipMemcpyDefault, s));
        sync_needed |= ptr_kind(sf_out, b->device) == PTR_HOST;
    }
    if (sync_needed) HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

extern "C" int mp3d_batch_synth_only(mp3d_batch *b, const float *xr, const uint8_t *block_type, const uint8_t *mixed,
                                     int n, int F, int nch, int hz, int16_t *pcm, void *hip_stream) {
    if (!b || !xr || !block_type || !mixed || !pcm || n <= 0 || F <= 0 || (nch != 1 && nch != 2)) return MP3D_E_ARG;
    if (n > b->max_streams || F > b->max_frames) return MP3D_E_CAPACITY;
    int sr = hz == 44100 ? 0 : hz == 48000 ? 1 : hz == 32000 ? 2 : -1;
    if (sr < 0) return MP3D_E_ARG;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    bool sync_needed = false;
    size_t nx = (size_t)n * F * 2 * nch;
    const float *dxr = xr;
    const uint8_t *dbt = block_type, *dmx = mixed;
    if (!is_device_ptr(xr, b->device) || !is_device_ptr(block_type, b->device) || !is_device_ptr(mixed, b->device)) {
        size_t need = nx * 576 * sizeof(float) + 2 * nx + 64;
        RCCHK(b->d_xr.grow(b, need));
        uint8_t *base = b->d_xr;
        HIPCHK(hipMemcpyAsync(base, xr, nx * 576 * sizeof(float), hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(base + nx * 576 * sizeof(float), block_type, nx, hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(base + nx * 576 * sizeof(float) + nx, mixed, nx, hipMemcpyDefault, s));
        dxr = (const float *)base;
        dbt = base + nx * 576 * sizeof(float);
        dmx = dbt + nx;
        sync_needed = true;
    }
    size_t pcm_bytes = (size_t)n * F * 2304 * sizeof(int16_t);
    int16_t *dpcm = pcm;
    const PtrKind pk = ptr_kind(pcm, b->device);
    const bool pcm_host = pk != PTR_DEV; /* host, or another GPU's (staged like host) */
    if (pcm_host) {
        RCCHK(b->d_pcm.grow(b, pcm_bytes));
        dpcm = b->d_pcm;
        /* mono rows are half written: the rest keeps the caller's bytes */
        if (pk == PTR_OTHER_DEV || nch == 1) HIPCHK(hipMemcpyAsync(dpcm, pcm, pcm_bytes, hipMemcpyDefault, s));
    }
    DeviceCtx &dc = g_dev[b->device];
    for (int i = 0; i < 3; i++) RCCHK(core_mark(b, i, s)); /* no front half: its events back to back */
    /* few streams: frame-parallel segments (seg_frames; one warm-up frame
     * each, so >= 4 frames per segment: warm-up overhead <= 25 %) */
    const int seg_len = seg_frames(n, F, dc.n_cu, 4);
    TailPlan tp;
    RCCHK(tail_plan(b, n, F, seg_len, s, &tp));
    RCCHK(core_launch(b, 3, s, [&] {
        launch_synth_xr(dxr, dbt, dmx, dc.tables, b->st, dpcm, n, F, nch, sr, seg_len, tp.out, tp.in, s);
    }));
    tail_commit(b, n, F, seg_len, tp);
    if (pcm_host) {
        HIPCHK(hipMemcpyAsync(pcm, dpcm, pcm_bytes, hipMemcpyDefault, s));
        sync_needed = sync_needed || pk == PTR_HOST;
    }
    if (sync_needed) HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

static void tag_to_info(uint32_t tag, uint32_t frames, int kind, mp3d_stream_info *o) {
    memset(o, 0, sizeof(*o));
    o->has_tag = (tag & MP3D_TAG_SEEN) != 0;
    o->has_lame = (tag & MP3D_TAG_LAME) != 0;
    o->total_frames = (tag & MP3D_TAG_FRAMES) ? (int)frames : -1;
    o->end_sample = -1;
    if (o->has_lame) {
        o->enc_delay = (int)((tag >> 12) & 0xFFFu);
        o->enc_padding = (int)(tag & 0xFFFu);
        o->skip_samples = o->enc_delay + 529; /* FFmpeg: start_pad + 528 + 1 */
        if (o->total_frames > 0) o->end_sample = (long long)o->total_frames * (kind == 2 ? 576 : 1152) + 529 - o->enc_padding;
    }
}

extern "C" int mp3d_batch_stream_info(mp3d_batch *b, int n, mp3d_stream_info *out) {
    if (!b || !out || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    HIPCHK(hipSetDevice(b->device));
    /* StreamState tag_info, tag_frames, kind: three consecutive words */
    std::vector<uint32_t> tag((size_t)n * 3);
    RCCHK(own_after_last(b)); /* after the handle's last call, on any stream */
    HIPCHK(hipMemcpy2DAsync(tag.data(), 3 * sizeof(uint32_t), &b->st[0].tag_info, sizeof(StreamState),
                            3 * sizeof(uint32_t), n, hipMemcpyDeviceToHost, b->own));
    HIPCHK(hipStreamSynchronize(b->own));
    for (int i = 0; i < n; i++) tag_to_info(tag[3 * i], tag[3 * i + 1], (int)tag[3 * i + 2], &out[i]);
    return MP3D_OK;
}

/* ------------------------------------------------------------------------ */
/* Per-stream state save / restore                                          */
/* ------------------------------------------------------------------------ */
extern "C" size_t mp3d_state_bytes(void) { return sizeof(StreamState); }

/* every blob must carry this build's format stamp (StreamState.fmt): a blob
 * of another state format would decode with wrong history.  Reads only the
 * blob (a device blob through the handle's own stream, after its last call);
 * the handle's state is untouched. */
int mp3d::blob_check(mp3d_batch *b, int n, const void *src) {
    std::vector<uint32_t> fmt((size_t)n);
    const uint8_t *f0 = (const uint8_t *)src + offsetof(StreamState, fmt);
    if (ptr_kind(src, b->device) == PTR_HOST) {
        for (int i = 0; i < n; i++) memcpy(&fmt[i], f0 + sizeof(StreamState) * (size_t)i, sizeof(uint32_t));
    } else {
        HIPCHK(hipSetDevice(b->device));
        RCCHK(own_after_last(b));
        HIPCHK(hipMemcpy2DAsync(fmt.data(), sizeof(uint32_t), f0, sizeof(StreamState), sizeof(uint32_t), (size_t)n,
                                hipMemcpyDefault, b->own));
        HIPCHK(hipStreamSynchronize(b->own));
    }
    for (int i = 0; i < n; i++)
        if (fmt[i] != MP3D_STATE_FMT) return MP3D_E_ARG;
    return MP3D_OK;
}

static int state_copy(mp3d_batch *b, int first, int n, void *dst, const void *src, bool out) {
    if (!b || !(out ? dst : src) || first < 0 || n <= 0) return MP3D_E_ARG;
    if ((long long)first + n > b->max_streams) return MP3D_E_CAPACITY;
    if (!out) RCCHK(blob_check(b, n, src)); /* before anything is written */
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = b->own;
    RCCHK(own_after_last(b)); /* after the handle's last call, on any stream */
    RCCHK(flush_tail(b, s));
    StreamState *at = b->st + first;
    HIPCHK(hipMemcpyAsync(out ? dst : (void *)at, out ? (const void *)at : src, sizeof(StreamState) * (size_t)n,
                          hipMemcpyDefault, s));
    /* a restored state is a discontinuity: the slots' resamplers restart */
    if (!out && b->rs.st) HIPCHK(hipMemsetAsync(b->rs.st + first, 0, sizeof(RsState) * (size_t)n, s));
    if (!out) RCCHK(stages_restart(b, first, n, s));
    HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

extern "C" int mp3d_batch_get_state(mp3d_batch *b, int first, int n, void *buf) {
    return state_copy(b, first, n, buf, nullptr, true);
}

extern "C" int mp3d_batch_set_state(mp3d_batch *b, int first, int n, const void *buf) {
    return state_copy(b, first, n, nullptr, buf, false);
}

/* ------------------------------------------------------------------------ */
extern "C" const char *mp3d_strerror(int e) {
    switch (e) {
    case MP3D_OK: return "ok";
    case MP3D_E_ARG: return "bad argument";
    case MP3D_E_NO_DEVICE: return "no usable HIP device (MI355X required; no CPU fallback)";
    case MP3D_E_HIP: return "HIP runtime error";
    case MP3D_E_NOMEM: return "out of memory";
    case MP3D_E_CAPACITY: return "batch exceeds handle capacity";
    case MP3D_E_NEED_MORE: return "no complete frame in buffer";
    default: return "unknown error";
    }
}
extern "C" int mp3d_last_hip_error(void) { return g_last_hip; }
extern "C" int mp3d_abi_version(void) { return MP3D_ABI_VERSION; }

#ifdef MP3D_WG_LDS_POISON
/* libmp3d_wglds.so only (the build whose every workgroup fills its static
 * LDS at entry, MP3D_LDS_ENTRY): the positive control of that fill.  Leaves
 * 0x5A5A5A5A in the CUs' LDS, then runs n_groups probe workgroups
 * (k_wglds_probe) and copies what each found in its static LDS after the
 * entry fill to out_words[g * words ...]; words >= the return value of a
 * call with out_words = NULL (the probe's LDS size in words, rounded up).
 * Returns the probe's static LDS size in bytes as the device reports it. */
extern "C" __attribute__((visibility("default"))) int mp3d_debug_wglds_probe(int device, int n_groups,
                                                                             uint32_t *out_words, int words) {
    const int W = wglds_probe_words();
    if (!out_words) return W;
    if (n_groups <= 0 || n_groups > (1 << 16) || words < W) return MP3D_E_ARG;
    RCCHK(device_init(device));
    uint32_t *d = nullptr;
    const size_t n = (size_t)n_groups * (W + 1);
    HIPCHK(hipMalloc(&d, n * sizeof(uint32_t)));
    std::vector<uint32_t> h(n);
    hipError_t e = hipMemset(d, 0, n * sizeof(uint32_t));
    if (e == hipSuccess) {
        launch_wglds_probe(g_dev[device].n_cu, n_groups, d, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(h.data(), d, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(e);
    int bytes = (int)h[W];
    for (int g = 0; g < n_groups; g++) {
        memcpy(out_words + (size_t)g * words, &h[(size_t)g * (W + 1)], sizeof(uint32_t) * W);
        if ((int)h[(size_t)g * (W + 1) + W] != bytes) bytes = -1; /* (every workgroup reports the same size) */
    }
    return bytes < 0 ? MP3D_E_HIP : bytes;
}
#endif
