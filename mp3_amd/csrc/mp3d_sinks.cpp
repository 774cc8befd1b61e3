/*
 * mp3d_sinks.cpp -- the sinks behind a batch decode: the packed
 * uniform-rate PCM sink (filter design, per-stream windows) and the log-mel
 * feature sink on top of it.
 */
#include "mp3d_host.h"

using namespace mp3d;

/* ------------------------------------------------------------------------ */
/* Packed uniform-rate PCM sink (DESIGN.md "Packed PCM sink")                */
/* ------------------------------------------------------------------------ */
const int mp3d::RS_RATES[MP3D_RS_RATES] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000};
int mp3d::rs_rate_index(int hz) {
    for (int i = 0; i < MP3D_RS_RATES; i++)
        if (RS_RATES[i] == hz) return i;
    return -1;
}
static long long rs_gcd(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}
/* modified Bessel function I0 by its power series (x <= 9 here) */
static double rs_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}
void mp3d::rs_sizes(int in_hz, int out_hz, int *L, int *M, int *T) {
    if (in_hz == out_hz) {
        *L = *M = *T = 1;
        return;
    }
    const int g = (int)rs_gcd(in_hz, out_hz);
    *L = out_hz / g;
    *M = in_hz / g;
    /* W = 24 / r = 24 M / L when downsampling, else 24; T = 2 ceil(W) */
    *T = *L < *M ? 2 * (int)((24LL * *M + *L - 1) / *L) : 48;
}
/* the Kaiser-windowed sinc of include/mp3d.h, taps[L][T] (row stride ld) */
static void rs_design(int L, int M, int T, float *taps, int ld) {
    if (T == 1) {
        taps[0] = 1.0f;
        return;
    }
    const double r = L < M ? (double)L / M : 1.0, W = 24.0 / r, i0b = rs_i0(9.0);
    std::vector<double> h((size_t)T);
    for (int p = 0; p < L; p++) {
        double sum = 0.0;
        for (int j = 0; j < T; j++) {
            const double t = (double)p / L - (j - (T / 2 - 1));
            double w = 0.0;
            if (fabs(t) < W) w = rs_i0(9.0 * sqrt(1.0 - (t / W) * (t / W))) / i0b;
            const double x = 0.88 * r * t;
            const double sinc = x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
            h[j] = 0.88 * r * sinc * w;
            sum += h[j];
        }
        for (int j = 0; j < T; j++) taps[(size_t)p * ld + j] = (float)(h[j] / sum);
    }
}

extern "C" long long mp3d_resample_filter(int in_hz, int out_hz, int *L, int *M, int *T, float *taps, size_t cap) {
    if (rs_rate_index(in_hz) < 0 || rs_rate_index(out_hz) < 0) return MP3D_E_ARG;
    int l, m, t;
    rs_sizes(in_hz, out_hz, &l, &m, &t);
    if (L) *L = l;
    if (M) *M = m;
    if (T) *T = t;
    const long long n = (long long)l * t;
    if (taps) {
        if ((long long)cap < n) return MP3D_E_ARG;
        rs_design(l, m, t, taps, t);
    }
    return n;
}

long long mp3d::rs_bound(int in_hz, int out_hz, long long frames) {
    int L, M, T;
    rs_sizes(in_hz, out_hz, &L, &M, &T);
    const long long N = frames * (in_hz >= 32000 ? 1152 : 576) + (T == 1 ? 0 : T / 2);
    return (N * L + M - 1) / M;
}

extern "C" long long mp3d_packed_max_samples(int out_hz, int frames, int min_in_hz) {
    if (rs_rate_index(out_hz) < 0 || frames < 0) return MP3D_E_ARG;
    long long best = 0;
    for (int hz : RS_RATES)
        if (hz >= min_in_hz) best = std::max(best, rs_bound(hz, out_hz, frames));
    return best;
}

/* the filters of one output rate: one per input rate; rows padded to 4
 * floats for 16-byte loads */
static void rs_build(int out_hz, int out_channels, RsCfg &cfg, std::vector<float> &tab) {
    cfg = RsCfg{};
    cfg.out_ch = out_channels;
    tab.clear();
    for (int i = 0; i < MP3D_RS_RATES; i++) {
        RsFilt &f = cfg.f[i];
        rs_sizes(RS_RATES[i], out_hz, &f.L, &f.M, &f.T);
        f.Tp = (f.T + 3) & ~3;
        f.pre = f.T == 1 ? 0 : f.T / 2 - 1;
        f.post = f.T == 1 ? 0 : f.T / 2;
        f.off = (int32_t)tab.size();
        tab.resize(tab.size() + (size_t)f.L * f.Tp, 0.0f);
        rs_design(f.L, f.M, f.T, tab.data() + f.off, f.Tp);
        /* a tile's input span is at most (tile - 1) M / L + 1 + T samples */
        long long tile = std::max<long long>(1, (long long)(MP3D_RS_SPAN - f.T - 2) * f.L / f.M);
        f.S = MP3D_RS_THREADS;
        if (f.T == MP3D_RS_UP_TAPS) {
            /* a thread's output stride: the multiple of L (<= 2048, or L) that
             * fills whole passes of the block best */
            double best = -1.0;
            for (int c = 1; c == 1 || c * f.L <= 2048; c++) {
                const int S = c * f.L, passes = (S + MP3D_RS_THREADS - 1) / MP3D_RS_THREADS;
                const double fill = (double)S / (passes * MP3D_RS_THREADS);
                if (fill > best + 1e-9) {
                    best = fill;
                    f.S = S;
                }
            }
            tile = std::min<long long>(tile, std::max(4096, 8 * f.S));
        }
        f.tile = (int32_t)tile;
    }
}

int RsFilters::upload(const mp3d_batch *b, int out_hz, int out_channels, hipStream_t s) {
    RsCfg c;
    std::vector<float> t;
    rs_build(out_hz, out_channels, c, t);
    hz = 0; /* none until the new ones are on the device */
    RCCHK(dcfg.grow(b, sizeof(RsCfg)));
    RCCHK(tab.grow(b, sizeof(float) * t.size()));
    HIPCHK(hipMemcpyAsync(dcfg, &c, sizeof(c), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(tab, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s)); /* (c and t are on this stack) */
    cfg = c;
    hz = out_hz;
    return MP3D_OK;
}

extern "C" int mp3d_batch_set_output(mp3d_batch *b, int out_hz, int out_channels) {
    if (!b) return MP3D_E_ARG;
    if (out_hz != 0 && (rs_rate_index(out_hz) < 0 || (out_channels != 1 && out_channels != 2))) return MP3D_E_ARG;
    RCCHK(set_begin(b));
    stages_off(b);
    mp3d_batch::PackedSink &k = b->rs;
    if (out_hz == 0) {
        k.off();
        return MP3D_OK;
    }
    const size_t ns = (size_t)b->max_streams;
    int r = k.st.grow(b, sizeof(RsState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(RsPlan) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    /* a change of the output format restarts every stream's resampler */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(RsState) * ns, b->own));
    if (!r) r = k.f.upload(b, out_hz, out_channels, b->own); /* (waits for the stream) */
    if (r) k.off();
    k.ch = r ? 0 : out_channels;
    k.tm.timed = false;
    return r;
}

int mp3d::deliver_rows(hipStream_t s, int n, size_t unit, const void *drows, long long dstride, void *rows,
                       long long stride, const int32_t *dcnt, int *count, bool rows_dev, bool cnt_dev) {
    if (rows_dev && cnt_dev) return MP3D_OK;
    std::vector<int32_t> hc((size_t)n);
    HIPCHK(hipMemcpyAsync(hc.data(), dcnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (!rows_dev)
        for (int i = 0; i < n; i++)
            if (hc[i] > 0)
                HIPCHK(hipMemcpyAsync((uint8_t *)rows + unit * (size_t)stride * i,
                                      (const uint8_t *)drows + unit * (size_t)dstride * i, unit * (size_t)hc[i],
                                      hipMemcpyDefault, s));
    if (!cnt_dev) HIPCHK(hipMemcpyAsync(count, hc.data(), sizeof(int32_t) * n, hipMemcpyDefault, s));
    HIPCHK(hipStreamSynchronize(s));
    return MP3D_OK;
}

extern "C" int mp3d_batch_decode_packed(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                        const uint32_t *sizes, int n, int F, void *out, int f32, long long out_stride,
                                        int *out_count, int flags, mp3d_frame_info *infos, void *hip_stream) {
    if (!b || !b->rs.f.hz || !out || !out_count || out_stride < 0 || (flags & ~(MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS)))
        return MP3D_E_ARG;
    if (!frames || !offsets || !sizes || n <= 0 || F <= 0) return MP3D_E_ARG;
    if (n > b->max_streams || F > b->max_frames) return MP3D_E_CAPACITY;
    HIPCHK(hipSetDevice(b->device));
    mp3d_batch::PackedSink &k = b->rs;
    const int oc = k.ch;
    const size_t eb = f32 ? sizeof(float) : sizeof(int16_t);
    /* blocks per stream: enough tiles for the longest output any input rate
     * can produce within the stride */
    const long long stride = std::min<long long>(out_stride, mp3d_packed_max_samples(k.f.hz, F, 0));
    long long tiles = 1;
    for (int i = 0; i < MP3D_RS_RATES; i++) {
        const long long most = std::min(stride, rs_bound(RS_RATES[i], k.f.hz, F));
        tiles = std::max(tiles, (most + k.f.cfg.f[i].tile - 1) / k.f.cfg.f[i].tile);
    }
    if (tiles * n > 0x7fffffffLL) return MP3D_E_CAPACITY;
    /* the kernel stores one sample frame (all channels) per instruction: a
     * device sink must be aligned to it (a host sink is filled by copies) */
    if (is_device_ptr(out, b->device) && (uintptr_t)out % (eb * oc)) return MP3D_E_ARG;
    RCCHK(k.rows.grow(b, sizeof(float) * 2304 * (size_t)n * F));
    RCCHK(k.prefix.grow(b, sizeof(int32_t) * (size_t)n * (F + 1)));
    const bool out_dev = is_device_ptr(out, b->device), cnt_dev = is_device_ptr(out_count, b->device);
    if (!out_dev) RCCHK(k.out.grow(b, eb * oc * (size_t)stride * n + 16));
    /* the decode itself: the float32 path into the handle's rows */
    DecodeCall c;
    c.frames = frames, c.offsets = offsets, c.sizes = sizes, c.n = n, c.F = F;
    c.pcm = k.rows, c.f32 = true, c.infos = infos, c.hip_stream = hip_stream;
    RCCHK(batch_decode(b, c));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    CallEnd done{b, s};
    const mp3d_frame_info *dinf = infos && is_device_ptr(infos, b->device) ? infos : b->d_infos.p;
    void *dout = out_dev ? out : k.out.p;
    int32_t *dcnt = cnt_dev ? (int32_t *)out_count : k.cnt.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_resample(k.rows, dinf, k.st, b->st, k.f.dcfg, oc, k.f.tab, k.plan, k.prefix, dout, f32 != 0, dcnt, n, F,
                        out_dev ? out_stride : stride, (int)tiles, (flags & MP3D_PACK_FLUSH) ? 1 : 0,
                        (flags & MP3D_PACK_GAPLESS) ? 1 : 0, s);
    }));
    /* the caller's stride is its own, the staging buffer's is `stride` */
    return deliver_rows(s, n, eb * oc, dout, stride, out, out_stride, dcnt, out_count, out_dev, cnt_dev);
}

extern "C" int mp3d_batch_resample_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->rs.tm, us) : MP3D_E_ARG;
}

int mp3d::stage_inputs(mp3d_batch *b, mp3d_batch::Stage &k, const float *samples, long long stride, size_t frame,
                       const int *counts, int n, hipStream_t s, const float **dsmp, const int32_t **dcin, bool *host) {
    const size_t bytes = frame * (size_t)stride * n;
    *dsmp = samples;
    if (stride && !is_device_ptr(samples, b->device)) {
        RCCHK(k.smp.grow(b, bytes));
        HIPCHK(hipMemcpyAsync(k.smp, samples, bytes, hipMemcpyDefault, s));
        *dsmp = k.smp;
        *host = true;
    } else if (stride && (uintptr_t)samples % sizeof(float)) {
        return MP3D_E_ARG;
    }
    return caller_in(b, (const int32_t *)counts, n, k.cin, s, dcin, host);
}

int mp3d::decode_to_stage(mp3d_batch *b, mp3d_batch::Stage &k, const uint8_t *frames, const uint64_t *offsets,
                          const uint32_t *sizes, int n, int F, int flags, mp3d_frame_info *infos, void *hip_stream,
                          long long *S, hipStream_t *s) {
    if (flags & ~(MP3D_PACK_FLUSH | MP3D_PACK_GAPLESS)) return MP3D_E_ARG;
    if (!frames || !offsets || !sizes || n <= 0 || F <= 0) return MP3D_E_ARG;
    if (n > b->max_streams || F > b->max_frames) return MP3D_E_CAPACITY;
    HIPCHK(hipSetDevice(b->device));
    /* a stride no stream can exceed, counts on the device */
    *S = stage_stride(b, F);
    RCCHK(k.smp.grow(b, sizeof(float) * (size_t)*S * b->rs.ch * n));
    *s = hip_stream ? (hipStream_t)hip_stream : b->own;
    return mp3d_batch_decode_packed(b, frames, offsets, sizes, n, F, k.smp, 1, *S, k.cin, flags, infos, hip_stream);
}

/* RsWindow is the head of RsState, r follows it: one strided copy each way */
static_assert(offsetof(RsState, rate_i) == 0 && offsetof(RsState, fixed) == offsetof(RsWindow, fixed) &&
                  offsetof(RsState, lo) == offsetof(RsWindow, lo) && offsetof(RsState, hi) == offsetof(RsWindow, hi) &&
                  offsetof(RsState, r) == sizeof(RsWindow),
              "RsWindow must mirror the head of RsState");

extern "C" int mp3d_batch_set_window(mp3d_batch *b, int first, int n, const long long *lo, const long long *hi) {
    if (!b || !b->rs.f.hz || first < 0 || n <= 0 || (!lo && hi)) return MP3D_E_ARG;
    if ((long long)first + n > b->max_streams) return MP3D_E_CAPACITY;
    std::vector<RsWindow> w;
    if (lo) {
        w.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            const long long h = hi ? hi[i] : MP3D_WINDOW_NO_END;
            if (lo[i] < 0 || h < lo[i]) return MP3D_E_ARG; /* before anything is written */
            w[i] = RsWindow{0, 1, lo[i], h};
        }
    }
    return slots_set(b, [&](hipStream_t s) -> int {
        /* a window restart: the slots' resamplers and fed counts restart with it */
        HIPCHK(hipMemsetAsync(b->rs.st + first, 0, sizeof(RsState) * (size_t)n, s));
        RCCHK(stages_restart(b, first, n, s));
        if (lo)
            HIPCHK(hipMemcpy2DAsync(b->rs.st + first, sizeof(RsState), w.data(), sizeof(RsWindow), sizeof(RsWindow),
                                    (size_t)n, hipMemcpyHostToDevice, s));
        return MP3D_OK;
    });
}

extern "C" int mp3d_batch_sink_window(mp3d_batch *b, int first, int n, long long *lo, long long *hi, long long *fed) {
    if (!b || !b->rs.f.hz || first < 0 || n <= 0) return MP3D_E_ARG;
    if ((long long)first + n > b->max_streams) return MP3D_E_CAPACITY;
    struct Head {
        RsWindow w;
        int64_t r;
    };
    std::vector<Head> h((size_t)n);
    HIPCHK(hipSetDevice(b->device));
    RCCHK(own_after_last(b));
    HIPCHK(hipMemcpy2DAsync(h.data(), sizeof(Head), b->rs.st + first, sizeof(RsState), sizeof(Head), (size_t)n,
                            hipMemcpyDeviceToHost, b->own));
    HIPCHK(hipStreamSynchronize(b->own));
    for (int i = 0; i < n; i++) {
        if (lo) lo[i] = h[i].w.fixed ? h[i].w.lo : 0;
        if (hi) hi[i] = h[i].w.fixed ? h[i].w.hi : MP3D_WINDOW_NO_END;
        if (fed) fed[i] = h[i].r;
    }
    return MP3D_OK;
}

/* ------------------------------------------------------------------------ */
/* Log-mel feature sink (mp3d_features.h)              */
/* ------------------------------------------------------------------------ */
static double ft_mel(double f) { return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + log(f / 1000.0) * 27.0 / log(6.4); }
static double ft_hz(double m) { return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * exp((m - 15.0) * log(6.4) / 27.0); }

/* the Slaney filterbank of include/mp3d.h, fb[n_mels][201] */
static void ft_filterbank(int n_mels, float *fb) {
    std::vector<double> c((size_t)n_mels + 2);
    const double top = ft_mel(8000.0);
    for (int i = 0; i < n_mels + 2; i++) c[i] = ft_hz(i * top / (n_mels + 1));
    for (int j = 0; j < n_mels; j++)
        for (int k = 0; k < MP3D_FT_BINS; k++) {
            const double f = 40.0 * k;
            const double up = (f - c[j]) / (c[j + 1] - c[j]), down = (c[j + 2] - f) / (c[j + 2] - c[j + 1]);
            fb[(size_t)j * MP3D_FT_BINS + k] = (float)(std::max(0.0, std::min(up, down)) * 2.0 / (c[j + 2] - c[j]));
        }
}

extern "C" long long mp3d_mel_filterbank(int n_mels, float *fb, size_t cap) {
    if (n_mels < 1 || n_mels > MP3D_FT_MAX_MELS) return MP3D_E_ARG;
    const long long n = (long long)n_mels * MP3D_FT_BINS;
    if (fb) {
        if ((long long)cap < n) return MP3D_E_ARG;
        ft_filterbank(n_mels, fb);
    }
    return n;
}

/* the most frames S new samples can emit on top of a pending carry */
static long long ft_bound(long long S) { return (S + MP3D_FT_HALF + MP3D_FT_HOP - 1) / MP3D_FT_HOP + 1; }

extern "C" long long mp3d_feat_max_frames(int frames, int min_in_hz) {
    const long long S = mp3d_packed_max_samples(16000, frames, min_in_hz);
    if (S <= 0) return S;
    return ft_bound(S);
}

/* the transform's tables and the filterbank as ranges plus weights */
static int ft_build(int n_mels, int flags, FtTab &t) {
    memset(&t, 0, sizeof(t));
    for (int n = 0; n < MP3D_FT_WIN; n++) t.win[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / MP3D_FT_WIN));
    for (int m = 0; m < MP3D_FT_HALF; m++) {
        t.w200[m][0] = (float)cos(2.0 * M_PI * m / MP3D_FT_HALF);
        t.w200[m][1] = (float)-sin(2.0 * M_PI * m / MP3D_FT_HALF);
    }
    for (int k = 0; k < MP3D_FT_BINS; k++) {
        t.w400[k][0] = (float)cos(2.0 * M_PI * k / MP3D_FT_WIN);
        t.w400[k][1] = (float)-sin(2.0 * M_PI * k / MP3D_FT_WIN);
    }
    std::vector<float> fb((size_t)n_mels * MP3D_FT_BINS);
    ft_filterbank(n_mels, fb.data());
    int used = 0;
    for (int j = 0; j < n_mels; j++) {
        const float *row = fb.data() + (size_t)j * MP3D_FT_BINS;
        int lo = MP3D_FT_BINS, hi = -1;
        for (int k = 0; k < MP3D_FT_BINS; k++)
            if (row[k] != 0.0f) {
                lo = std::min(lo, k);
                hi = k;
            }
        const int len = hi < 0 ? 0 : hi - lo + 1;
        if (used + len > MP3D_FT_MAX_WTS) return MP3D_E_ARG;
        t.first[j] = len ? lo : 0;
        t.len[j] = len;
        t.off[j] = used;
        for (int i = 0; i < len; i++) t.wts[used + i] = row[lo + i];
        used += len;
    }
    t.n_mels = n_mels;
    t.log10 = (flags & MP3D_FEAT_LOG10) ? 1 : 0;
    return MP3D_OK;
}

extern "C" int mp3d_batch_set_features(mp3d_batch *b, int n_mels, int flags) {
    if (!b || n_mels < 0 || n_mels > MP3D_FT_MAX_MELS || (flags & ~MP3D_FEAT_LOG10)) return MP3D_E_ARG;
    if (n_mels && (b->rs.f.hz != 16000 || b->rs.ch != 1)) return MP3D_E_ARG;
    RCCHK(set_begin(b));
    mp3d_batch::FeatureSink &k = b->ft;
    if (n_mels == 0) {
        k.off();
        return MP3D_OK;
    }
    FtTab tab;
    RCCHK(ft_build(n_mels, flags, tab));
    const size_t ns = (size_t)b->max_streams;
    int r = k.tab.grow(b, sizeof(FtTab));
    if (!r) r = k.st.grow(b, sizeof(FtState) * ns);
    if (!r) r = k.plan.grow(b, sizeof(FtPlan) * ns);
    if (!r) r = k.cin.grow(b, sizeof(int32_t) * ns);
    if (!r) r = k.cnt.grow(b, sizeof(int32_t) * ns);
    if (!r) r = hip_rc(hipMemcpyAsync(k.tab, &tab, sizeof(tab), hipMemcpyHostToDevice, b->own));
    /* a change of the features restarts every stream's feature state */
    if (!r) r = hip_rc(hipMemsetAsync(k.st, 0, sizeof(FtState) * ns, b->own));
    r = set_end(b, k, r); /* (tab is on this stack) */
    k.mels = r ? 0 : n_mels;
    return r;
}

/* The feature stage on stream s: dsmp [n][sstride] samples and dcin [n]
 * counts are device memory; feat and feat_count are the caller's (host or
 * device).  Returns after the work is queued when both are device memory,
 * else when it is done. */
static int ft_run(mp3d_batch *b, const float *dsmp, const int32_t *dcin, long long sstride, int n, float *feat,
                  long long feat_stride, int *feat_count, int flags, hipStream_t s) {
    mp3d_batch::FeatureSink &k = b->ft;
    const bool out_dev = is_device_ptr(feat, b->device);
    /* blocks per stream: enough tiles for the most frames the stride admits */
    const long long stride = std::min(feat_stride, ft_bound(sstride));
    const long long tiles = std::max<long long>(1, (stride + MP3D_FT_TILE - 1) / MP3D_FT_TILE);
    if (tiles * n > 0x7fffffffLL) return MP3D_E_CAPACITY;
    if (out_dev && (uintptr_t)feat % sizeof(float)) return MP3D_E_ARG;
    CallerOut<int32_t> cnt;
    RCCHK(cnt.pick(b, (int32_t *)feat_count, k.cnt));
    if (!out_dev) RCCHK(k.out.grow(b, sizeof(float) * k.mels * (size_t)stride * n + 16));
    float *dout = out_dev ? feat : (float *)k.out.p;
    RCCHK(stage_launch(b, &k.tm, s, [&] {
        launch_features(dsmp, dcin, k.st, k.plan, k.tab, dout, cnt.dev, n, sstride, out_dev ? feat_stride : stride,
                        (int)tiles, (flags & MP3D_PACK_FLUSH) ? 1 : 0, s);
    }));
    return deliver_rows(s, n, sizeof(float) * k.mels, dout, stride, feat, feat_stride, cnt.dev, feat_count, out_dev,
                        !cnt.host);
}

extern "C" int mp3d_batch_decode_features(mp3d_batch *b, const uint8_t *frames, const uint64_t *offsets,
                                          const uint32_t *sizes, int n, int F, float *feat, long long feat_stride,
                                          int *feat_count, int flags, mp3d_frame_info *infos, void *hip_stream) {
    if (!b || !b->ft.mels || !feat || !feat_count || feat_stride < 0) return MP3D_E_ARG;
    long long S;
    hipStream_t s;
    RCCHK(decode_to_stage(b, b->ft, frames, offsets, sizes, n, F, flags, infos, hip_stream, &S, &s));
    CallEnd done{b, s};
    return ft_run(b, b->ft.smp, b->ft.cin, S, n, feat, feat_stride, feat_count, flags, s);
}

extern "C" int mp3d_batch_features(mp3d_batch *b, const float *samples, long long sample_stride, const int *counts, int n,
                                   float *feat, long long feat_stride, int *feat_count, int flags, void *hip_stream) {
    if (!b || !b->ft.mels || !counts || !feat || !feat_count || sample_stride < 0 || feat_stride < 0 ||
        (flags & ~MP3D_PACK_FLUSH))
        return MP3D_E_ARG;
    if ((!samples && sample_stride) || n <= 0) return MP3D_E_ARG;
    if (n > b->max_streams) return MP3D_E_CAPACITY;
    if (sample_stride > 0x7fffffffLL) return MP3D_E_ARG; /* counts are int */
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : b->own;
    RCCHK(call_begin(b, s));
    CallEnd done{b, s};
    const float *dsmp;
    const int32_t *dcin;
    bool host_in = false;
    RCCHK(stage_inputs(b, b->ft, samples, sample_stride, sizeof(float), counts, n, s, &dsmp, &dcin, &host_in));
    RCCHK(ft_run(b, dsmp, dcin, sample_stride, n, feat, feat_stride, feat_count, flags, s));
    if (host_in) HIPCHK(hipStreamSynchronize(s)); /* the caller's host arrays are read until here */
    return MP3D_OK;
}

extern "C" int mp3d_batch_feature_time(mp3d_batch *b, float *us) {
    return b ? stage_time(b, b->ft.tm, us) : MP3D_E_ARG;
}
