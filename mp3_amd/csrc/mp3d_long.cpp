/*
 * mp3d_long.cpp -- one long stream decoded as frame-parallel segments
 * (SURVEY.md §8(f) row 2): mp3d_long_plan, mp3d_batch_decode_long, and the
 * same into the packed sink's format (mp3d_batch_decode_long_packed).
 */
#include "mp3d_host.h"

using namespace mp3d;

extern "C" int mp3d_long_plan(const uint8_t *data, size_t bytes, int L, long long max_frames, uint64_t *frame_off,
                              long long *seg_start, long long *n_frames, int *max_warmup) {
    if (!data || L <= 0 || max_frames < 0 || !n_frames) return MP3D_E_ARG;
    std::vector<uint64_t> off;
    std::vector<long long> a;
    int wmax = 0;
    *n_frames = 0;
    RCCHK(long_plan(data, bytes, L, max_frames, off, a, &wmax));
    *n_frames = (long long)off.size();
    if (frame_off) std::copy(off.begin(), off.end(), frame_off);
    if (seg_start) std::copy(a.begin(), a.end(), seg_start);
    if (max_warmup) *max_warmup = wmax;
    return MP3D_OK;
}

/* The segmented decode of one stream, shared by mp3d_batch_decode_long and
 * mp3d_batch_decode_long_packed: plan() walks the frames, open() stages the
 * input and allocates the scratch, decode_chunk(k0) decodes segments
 * [k0, k0 + ns) as virtual streams into seg_pcm [ns][F][2304] (infos in
 * b->d_infos), the destructor waits and gives the handle back as it was. */
struct LongRun {
    mp3d_batch *b;
    /* the virtual streams decode on a state array of their own: the handle's
     * per-stream state (reservoir, overlap, FIFO, tag) is left as it was */
    StreamState *own_st;
    hipStream_t s;
    std::vector<uint8_t> host_copy;
    std::vector<uint64_t> off;
    std::vector<long long> a;
    std::vector<int> a32;
    const uint8_t *data = nullptr, *hp = nullptr, *din = nullptr;
    size_t bytes = 0, row = 0;
    long long N = 0, K = 0;
    int L = 0, F = 0, chunk = 0;
    bool f32 = false, swapped = false;
    DevBuf<void> seg_pcm; /* (the scratch is freed after the destructor's wait) */
    DevBuf<StreamState> seg_st;
    DevBuf<int> d_a;

    explicit LongRun(mp3d_batch *b_) : b(b_), own_st(b_->st), s(b_->own) {}
    ~LongRun() {
        (void)hipStreamSynchronize(s);
        b->st = own_st;
        if (swapped) b->tail_live = -1; /* a tail left by the segments belongs to the scratch states */
    }
    /* the frame walk (on the host: a device stream is copied); N = 0: no frame */
    int plan(const uint8_t *data_, size_t bytes_, int L_, long long max_frames) {
        data = hp = data_;
        bytes = bytes_;
        L = L_;
        if (ptr_kind(data, b->device) != PTR_HOST) { /* any GPU's: the walk needs a host copy */
            host_copy.resize(bytes);
            HIPCHK(hipMemcpy(host_copy.data(), data, bytes, hipMemcpyDefault));
            hp = host_copy.data();
        }
        int wmax = 0;
        RCCHK(long_plan(hp, bytes, L, max_frames, off, a, &wmax));
        N = (long long)off.size();
        K = (long long)a.size();
        F = L + wmax;
        return MP3D_OK;
    }
    /* input staged, scratch allocated; chunk_ = segments per batch call */
    int open(bool f32_, int chunk_) {
        if (F > b->max_frames) return MP3D_E_CAPACITY;
        f32 = f32_;
        chunk = chunk_;
        row = 2304 * (f32 ? sizeof(float) : sizeof(int16_t));
        RCCHK(own_after_last(b));
        RCCHK(flush_tail(b, s)); /* before b->st points at the scratch states */
        din = data;
        if (!is_device_ptr(data, b->device)) { /* host or another GPU's: staged */
            RCCHK(b->d_in.grow(b, bytes + 64));
            HIPCHK(hipMemcpyAsync(b->d_in, data, bytes, hipMemcpyDefault, s));
            din = b->d_in;
        }
        const size_t ns = (size_t)std::min<long long>(chunk, K);
        RCCHK(seg_pcm.grow(b, ns * F * row));
        RCCHK(seg_st.grow(b, sizeof(StreamState) * ns));
        b->st = seg_st;
        swapped = true;
        RCCHK(d_a.grow(b, sizeof(int) * K));
        a32.assign(a.begin(), a.end());
        HIPCHK(hipMemcpyAsync(d_a, a32.data(), sizeof(int) * K, hipMemcpyHostToDevice, s));
        return MP3D_OK;
    }
    int segments(long long k0) const { return (int)std::min<long long>(chunk, K - k0); }
    int decode_chunk(long long k0) {
        const int ns = segments(k0);
        std::vector<uint64_t> so(ns);
        std::vector<uint32_t> ss(ns);
        for (int i = 0; i < ns; i++) {
            const long long k = k0 + i, e = std::min(N, (k + 1) * L);
            so[i] = k == 0 ? 0 : off[a[k]];
            ss[i] = (uint32_t)((e < N ? off[e] : bytes) - so[i]);
        }
        /* fresh decoder state for every virtual stream */
        HIPCHK(state_clear(b->st, ns, s));
        b->tail_live = -1; /* fresh states: no tail of the previous chunk */
        DecodeCall c; /* no infos for the caller: they stay in b->d_infos */
        c.frames = din, c.offsets = so.data(), c.sizes = ss.data(), c.n = ns, c.F = F;
        c.pcm = seg_pcm, c.f32 = f32, c.hip_stream = s;
        return batch_decode(b, c);
    }
};

extern "C" int mp3d_batch_decode_long(mp3d_batch *b, const uint8_t *data, size_t bytes, int L, void *pcm, int f32,
                                      long long max_frames, mp3d_frame_info *infos, long long *n_frames,
                                      mp3d_stream_info *sinfo) {
    if (!b || !data || !pcm || L <= 0 || max_frames <= 0 || !n_frames) return MP3D_E_ARG;
    *n_frames = 0;
    HIPCHK(hipSetDevice(b->device));
    const bool pcm_dev = is_device_ptr(pcm, b->device), inf_dev = infos && is_device_ptr(infos, b->device);
    /* the device images of a host pcm / infos: declared before R, so they are
     * freed after its destructor has waited for the stream */
    DevBuf<void> out_pcm;
    DevBuf<mp3d_frame_info> out_inf;
    LongRun R(b);
    RCCHK(R.plan(data, bytes, L, max_frames));
    const long long N = R.N;
    *n_frames = N;
    if (N == 0) return MP3D_OK;
    hipStream_t s = R.s;
    RCCHK(R.open(f32 != 0, b->max_streams));
    const size_t row = R.row;
    if (!pcm_dev) RCCHK(out_pcm.grow(b, (size_t)N * row));
    if (infos && !inf_dev) RCCHK(out_inf.grow(b, sizeof(mp3d_frame_info) * (size_t)N));
    void *dpcm = pcm_dev ? pcm : out_pcm.p;
    mp3d_frame_info *dinf = inf_dev ? infos : out_inf.p; /* (null without infos) */
    for (long long k0 = 0; k0 < R.K; k0 += R.chunk) {
        const int ns = R.segments(k0);
        RCCHK(R.decode_chunk(k0));
        if (k0 == 0 && sinfo) RCCHK(mp3d_batch_stream_info(b, 1, sinfo));
        const long long j0 = k0 * L, j1 = std::min(N, (k0 + ns) * L);
        launch_gather_frames(R.seg_pcm, (uint8_t *)dpcm + (size_t)j0 * row, b->d_infos, dinf ? dinf + j0 : nullptr,
                             R.d_a + k0, L, R.F, (int)k0, (int)(j1 - j0), (int)row, s);
        HIPCHK(hipGetLastError());
    }
    if (!pcm_dev) HIPCHK(hipMemcpyAsync(pcm, dpcm, (size_t)N * row, hipMemcpyDefault, s));
    if (infos && !inf_dev) HIPCHK(hipMemcpyAsync(infos, dinf, sizeof(mp3d_frame_info) * (size_t)N, hipMemcpyDefault, s));
    HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

/* ------------------------------------------------------------------------ */
/* One long stream into the packed sink's format      */
/* ------------------------------------------------------------------------ */
extern "C" long long mp3d_long_packed_bound(const uint8_t *data, size_t bytes, int out_hz) {
    if (!data || rs_rate_index(out_hz) < 0 || ptr_kind(data, 0) != PTR_HOST) return MP3D_E_ARG;
    std::vector<uint64_t> off;
    std::vector<uint32_t> pay;
    walk_frames(data, bytes, off, pay);
    if (off.empty()) return 0;
    const uint8_t *h = data + off[0];
    const int ver = (h[1] >> 3) & 3, si = (h[2] >> 2) & 3;
    const int hz = (int)MP3D_SAMPLE_RATE[si + (ver == 3 ? 0 : ver == 2 ? 3 : 6)];
    int L, M, T;
    rs_sizes(hz, out_hz, &L, &M, &T);
    const long long n = (long long)off.size() * (host_frame_kind(h) == 1 ? 1152 : 576);
    return (n * L + M - 1) / M;
}

extern "C" int mp3d_batch_decode_long_packed(mp3d_batch *b, const uint8_t *data, size_t bytes, int L, int out_hz,
                                             int out_channels, void *out, int f32, long long out_cap,
                                             long long *out_samples, int flags, mp3d_stream_info *sinfo, int *in_hz) {
    if (!b || !data || !out_samples || L <= 0 || rs_rate_index(out_hz) < 0 || (out_channels != 1 && out_channels != 2) ||
        out_cap < 0 || (!out && out_cap > 0) || (flags & ~MP3D_LONG_GAPLESS))
        return MP3D_E_ARG;
    *out_samples = 0;
    if (in_hz) *in_hz = 0;
    HIPCHK(hipSetDevice(b->device));
    const int oc = out_channels;
    const size_t eb = (f32 ? sizeof(float) : sizeof(int16_t)) * (size_t)oc; /* one sample frame */
    const bool out_dev = is_device_ptr(out, b->device);
    /* the kernel stores one sample frame per instruction, as the packed sink */
    if (out_dev && (uintptr_t)out % eb) return MP3D_E_ARG;
    /* a chunk's input count and its prefix are 32-bit */
    const long long lim = 0x7fffffffLL / (1152LL * L);
    if (lim < 1) return MP3D_E_CAPACITY;
    /* the call's scratch: declared before R, so it is freed after R's
     * destructor has waited for the stream */
    DevBuf<RsLong> d_st;
    DevBuf<int32_t> d_prefix;
    DevBuf<void> d_out; /* the device image of a host out */
    LongRun R(b);
    RCCHK(R.plan(data, bytes, L, 0x7fffffffffffffffLL));
    if (R.N == 0) return MP3D_OK;
    hipStream_t s = R.s;
    RCCHK(R.open(true, (int)std::min<long long>(b->max_streams, lim)));
    /* the filters: the sink's own when its rate matches, else those of the
     * last call of this kind (the sink's stay as they are) */
    const RsFilters *flt = &b->rs.f;
    if (flt->hz != out_hz) {
        flt = &b->lp;
        if (flt->hz != out_hz) RCCHK(b->lp.upload(b, out_hz, 0, s));
    }
    /* blocks per chunk: enough tiles for the most a chunk of any input rate
     * can emit (its inputs plus a pending tail) */
    const long long nf_max = std::min<long long>(R.N, (long long)R.chunk * L);
    long long tiles = 1, whole = 0;
    for (int i = 0; i < MP3D_RS_RATES; i++) {
        const long long most = rs_bound(RS_RATES[i], out_hz, nf_max) + 1;
        tiles = std::max(tiles, (most + flt->cfg.f[i].tile - 1) / flt->cfg.f[i].tile);
        whole = std::max(whole, rs_bound(RS_RATES[i], out_hz, R.N));
    }
    if (tiles > 0x7fffffffLL) return MP3D_E_CAPACITY;
    const long long cap = out_dev ? out_cap : std::min(out_cap, whole);
    RCCHK(d_st.grow(b, sizeof(RsLong)));
    RCCHK(d_prefix.grow(b, sizeof(int32_t) * (size_t)(nf_max + 1)));
    if (!out_dev && cap > 0) RCCHK(d_out.grow(b, eb * (size_t)cap));
    HIPCHK(hipMemsetAsync(d_st, 0, sizeof(RsLong), s)); /* the stream's start */
    void *dout = out_dev ? out : d_out.p;
    for (long long k0 = 0; k0 < R.K; k0 += R.chunk) {
        const int ns = R.segments(k0);
        RCCHK(R.decode_chunk(k0));
        if (k0 == 0 && sinfo) RCCHK(mp3d_batch_stream_info(b, 1, sinfo));
        const long long j0 = k0 * L, j1 = std::min(R.N, (k0 + ns) * L);
        /* (the tag words of virtual stream 0 are read by the first chunk's
         * plan, before the next chunk clears the states; mp3d_batch_resample_time:
         * the last chunk's stage) */
        RCCHK(stage_launch(b, &b->rs.tm, s, [&] {
            launch_resample_long((const float *)R.seg_pcm.p, b->d_infos, R.d_a + k0, &R.seg_st[0].tag_info, flt->dcfg,
                                 oc, flt->tab, d_st, d_prefix, dout, f32 != 0, cap, L, R.F, (int)k0, (int)(j1 - j0),
                                 (int)tiles, k0 == 0, k0 + ns >= R.K, (flags & MP3D_LONG_GAPLESS) ? 1 : 0, s);
        }));
    }
    RsLong end;
    HIPCHK(hipMemcpyAsync(&end, d_st, offsetof(RsLong, hist), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *out_samples = end.m1;
    if (in_hz) *in_hz = end.rate_i ? RS_RATES[end.rate_i - 1] : 0;
    const long long wrote = std::min<long long>(end.m1, cap);
    if (!out_dev && wrote > 0) HIPCHK(hipMemcpy(out, d_out, eb * (size_t)wrote, hipMemcpyDefault));
    return end.m1 > out_cap ? MP3D_E_CAPACITY : MP3D_OK;
}
