/*
 * mp3d_launch.h -- the host-callable entry points of the kernel files, each
 * declared once.  Included by the host sources that call them and by the
 * .hip file that defines each, so the compiler checks every declaration
 * against its definition.
 */
#ifndef MP3D_LAUNCH_H
#define MP3D_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* (layouts: mp3d_internal.h, mp3d_resample.h, mp3d_features.h, mp3d_loudness.h, mp3d_normalize.h,
 * mp3d_stretch.h, mp3d_limiter.h, mp3d_segment.h, mp3d_eq.h, mp3d_pitch.h) */
struct StreamState; struct FrameRec; struct UnitMeta; struct DevTables;
struct RsState; struct RsCfg; struct RsPlan; struct RsLong;
struct FtState; struct FtPlan; struct FtTab;
struct LdState; struct LdPlan; struct LdTab;
struct TpState; struct TpPlan;
struct StState; struct StPlan;
struct LimState; struct LimPlan;
struct SgState; struct SgPlan;
struct EqState; struct EqPlan; struct EqTab;
struct PtState; struct PtPlan;

namespace mp3d {

/* ---- mp3d_demux.hip ---- */
/* the frame-size table into the demux kernels' constant memory */
hipError_t upload_demux_constants(const uint16_t *frame_bytes);
/* k_walk + k_mdcopy (wide) or one k_demux wave per stream: headers, side info, main-data gather */
void launch_demux(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *md,
                  const uint64_t *md_off, StreamState *st, FrameRec *rec, uint64_t *sideu, void *infos, int n_streams,
                  int F, int opts, bool wide, uint32_t *fam, uint32_t seq, hipStream_t strm);
/* k_demux_fp: one stream's run of F pre-located frames (fo: host array of their offsets) */
void launch_demux_fp(const uint8_t *in, uint32_t len, const uint32_t *fo, uint8_t *md, StreamState *st,
                     const float *tail_in, StreamState *snap, FrameRec *rec, uint64_t *sideu, void *infos, int F,
                     int opts, hipStream_t strm);

/* ---- mp3d_huffman.hip ---- */
/* k_huffman_wave (one unit per wave) or k_rank + k_huffman (one unit per lane) */
void launch_huffman(const uint8_t *md, const uint64_t *md_off, const FrameRec *rec, const uint64_t *sideu,
                    const DevTables *tab, int16_t *is_buf, UnitMeta *meta, int n_streams, int F, int n_cu, bool wave,
                    uint32_t *work, uint32_t *rank, hipStream_t strm);

/* ---- mp3d_synth.hip ---- */
/* the long windows, intensity ratios and 2^(i/4) into k_synth's constant memory */
hipError_t upload_synth_constants(const float *win36, const float *is_ratio, const float *pow2q, const float *is_lsf);
/* the frame-size table into k_frame's constant memory */
hipError_t upload_frame_constants(const uint16_t *frame_bytes);
/* k_frame: one frame of one stream, demux to PCM in one launch; writes seq to *done last */
void launch_frame(const uint8_t *in_host, uint32_t in_have, const uint64_t *in_off, const uint32_t *in_len,
                  uint8_t *md, const uint64_t *md_off, StreamState *st, FrameRec *rec, uint64_t *sideu, void *infos,
                  int opts, const DevTables *tab, int16_t *is_buf, UnitMeta *meta, void *pcm, bool f32, bool lsf,
                  uint32_t *done, uint32_t seq, hipStream_t strm);
/* k_synth: requantize to PCM, the family variants in kinds, in segments of seg_len frames; longpath: all-long
 * M/S granules take phase Q's and the alias step's straight-line path (off: every granule the general one) */
void launch_synth(const FrameRec *rec, const int16_t *is_buf, const UnitMeta *meta, const DevTables *tab,
                  StreamState *st, void *pcm, bool f32, int n_streams, int F, int kinds, int seg_len, float *st_tail,
                  const float *st_tail_in, const uint32_t *fam, uint32_t seq, int n_cu, bool longpath,
                  hipStream_t strm);
/* k_synth from caller-supplied spectra (mp3d_batch_synth_only) */
void launch_synth_xr(const float *xr, const uint8_t *bt, const uint8_t *mixed, const DevTables *tab, StreamState *st,
                     int16_t *pcm, int n_streams, int F, int nch, int sr, int seg_len, float *st_tail,
                     const float *st_tail_in, hipStream_t strm);
/* MP3D_DEBUG_POISON: fill the whole LDS of every CU with 0xFF */
void launch_lds_poison(int n_cu, hipStream_t strm);
/* k_gather_frames: the segments' own frames (after each one's a[k] warm-up rows) to consecutive rows */
void launch_gather_frames(const void *src, void *dst, const void *isrc, void *idst, const int *a, int L, int F, int k0,
                          int n_out, int bytes_per_row, hipStream_t strm);
#ifdef MP3D_WG_LDS_POISON
/* the probe kernel's static LDS size in words */
int wglds_probe_words();
/* leave a pattern in the CUs' LDS, then n_groups probe workgroups report what they find */
void launch_wglds_probe(int n_cu, int n_groups, uint32_t *out, hipStream_t strm);
#endif

/* ---- mp3d_resample.hip ---- */
/* k_rs_plan + k_rs_filter + k_rs_update: a batch's float rows to packed PCM at one rate */
void launch_resample(const float *rows, const void *infos, RsState *st, const StreamState *sst, const RsCfg *cfg,
                     int out_ch, const float *tab, RsPlan *plan, int32_t *prefix, void *out, bool f32,
                     int32_t *out_count, int n, int F, long long stride, int tiles, int flush, int gapless,
                     hipStream_t strm);
/* the same for one chunk of a long stream's segments (mp3d_batch_decode_long_packed) */
void launch_resample_long(const float *rows, const void *infos, const int *a, const uint32_t *tag, const RsCfg *cfg,
                          int out_ch, const float *tab, RsLong *st, int32_t *prefix, void *out, bool f32, long long cap,
                          int L, int F, int k0, int n_out, int tiles, int first, int last, int gapless, hipStream_t strm);

/* ---- mp3d_features.hip ---- */
/* k_ft_plan + k_ft_transform + k_ft_update: 16 kHz mono samples to log-mel frames */
void launch_features(const float *samples, const int32_t *counts, FtState *st, FtPlan *plan, const FtTab *tab, float *feat,
                     int32_t *feat_count, int n, long long sample_stride, long long feat_stride, int tiles, int flush,
                     hipStream_t strm);

/* ---- mp3d_loudness.hip ---- */
/* k_ld_plan + k_ld_local + k_ld_carry + k_ld_energy + k_ld_finish: packed float32 samples to 100 ms block energies */
void launch_loudness(const float *samples, const int32_t *counts, LdState *st, LdPlan *plan, const LdTab *tab, int H,
                     int ch, double *tz, double *entry, double *part, float *tpeak, double *endst, float *blocks,
                     int32_t *block_count, float *peak, int n, long long sample_stride, long long block_stride,
                     int tiles, int flush, hipStream_t strm);
/* k_ld_gate: rows of block energies to gated integrated loudness */
void launch_loudness_gate(const float *blocks, long long block_stride, const int32_t *counts, float *lufs, int n,
                          hipStream_t strm);

/* ---- mp3d_normalize.hip ---- */
/* k_tp_plan + k_tp_peak + k_tp_finish: packed float32 samples to the 4x oversampled peak of each stream */
void launch_true_peak(const float *samples, const int32_t *counts, TpState *st, TpPlan *plan, const float *taps,
                      float *tilepk, float *tpeak, int n, long long sample_stride, int ch, int tiles, int flush,
                      hipStream_t strm);
/* k_gain_calc: loudness and true peak (or null) to the normalisation gain; c = 10^(max_dbtp / 20) */
void launch_gain_calc(const float *lufs, const float *tpeak, float *gain, int n, double target, double c,
                      hipStream_t strm);
/* k_gain_apply: packed float32 samples times their stream's gain, as float32 or int16; ccnt: the clamped counts */
void launch_gain_apply(const float *samples, const int32_t *counts, const float *gain, void *out, int32_t *ccnt,
                       bool f32, int ch, int n, long long sample_stride, int chunks, hipStream_t strm);

/* ---- mp3d_stretch.hip ---- */
/* k_st_plan + k_st_blocks: packed float32 samples to the same signal at each stream's tempo (num, den pairs) */
void launch_stretch(const float *samples, const int32_t *counts, StState *st, const int32_t *tempo, StPlan *plan,
                    const float *w, float *out, int32_t *out_count, int n, long long sample_stride,
                    long long out_stride, int H, int ch, int flush, hipStream_t strm);

/* ---- mp3d_limiter.hip ---- */
/* k_lim_plan + k_lim_tile + k_lim_carry: packed float32 samples times gain[s] (null: 1) and the limiter's gain
 * envelope under the ceiling c to float32 or int16; tilemin holds n * tiles floats, gr may be null */
void launch_limiter(const float *samples, const int32_t *counts, LimState *st, LimPlan *plan, const float *taps,
                    const float *gain, void *out, int32_t *out_count, float *tilemin, float *gr, bool f32, int ch, int n,
                    long long sample_stride, long long out_stride, int tiles, int A, float c, int flush,
                    hipStream_t strm);

/* ---- mp3d_segment.hip ---- */
/* k_sg_plan + k_sg_energy + k_sg_emit: packed float32 samples to the sample ranges of their speech segments; part
 * holds n words, bits n * tiles (a word per tile of MP3D_SG_TILE hops), seg n * seg_stride pairs */
void launch_segments(const float *samples, const int32_t *counts, SgState *st, SgPlan *plan, const uint64_t *thr,
                     uint64_t *part, uint64_t *bits, long long *seg, int32_t *seg_count, int ch, int n,
                     long long sample_stride, long long seg_stride, int tiles, int H, int P, int S, int pad, int flush,
                     hipStream_t strm);

/* ---- mp3d_eq.hip ---- */
/* k_eq_plan + k_eq_local + k_eq_carry + k_eq_apply: packed float32 samples through the handle's biquad cascade to
 * float32; K sections; tpow holds the cascade's A^(TILE t), tz and entry n * tiles * MP3D_EQ_TSTRIDE doubles each */
void launch_eq(const float *samples, const int32_t *counts, EqState *st, EqPlan *plan, const EqTab *tab,
               const double *tpow, double *tz, double *entry, float *out, int32_t *out_count, int K, int ch, int n,
               long long sample_stride, long long out_stride, int tiles, int flush, hipStream_t strm);

/* ---- mp3d_pitch.hip ---- */
/* k_pt_plan + k_pt_frames + k_pt_update: packed float32 samples to one 16-byte record (f0, periodicity, lag,
 * shift) per 10 ms frame; rec holds n * pitch_stride records; T = tmax + 1 lags over a window of 2 H samples */
void launch_pitch(const float *samples, const int32_t *counts, PtState *st, PtPlan *plan, void *rec,
                  int32_t *rec_count, int ch, int n, long long sample_stride, long long pitch_stride, int tiles, int fs,
                  int H, int T, int tmin, int theta, int flush, hipStream_t strm);

} // namespace mp3d

#endif
