"""mp3_amd -- MI355X-native batched MPEG-1 Layer III decoder (Python host side).

Mirrors the C ABI of include/mp3d.h (the drop-in boundary for the reference
player's per-frame decode call):

  Decoder       per-frame decode (mp3d_decode_frame): bytes -> int16 PCM
  BatchDecoder  many concurrent streams on one GPU (mp3d_batch_*), inputs and
                outputs as numpy arrays (host) or torch tensors (device)

The compute path is the HIP library mp3_amd/libmp3d.so; there is no CPU
fallback.  Importing works without a GPU; creating a decoder does not.
library(path) selects another build of the library (the tests' debug build
libmp3d_wglds.so) for the decoders created inside the block.

The ctypes side -- structs, constants, the table of every export's signature
and the loader -- is mp3_amd/_abi.py; its names are re-exported here.
"""
import ctypes

import numpy as np

from ._abi import (ABI, EQ_BAND_DT, EQ_HIGH_PASS, EQ_HIGH_SHELF, EQ_LOW_PASS, EQ_LOW_SHELF,  # noqa: F401
                   EQ_MAX_BANDS, EQ_PEAK, EXPORTS, FEAT_LOG10, FRAME_F32, FRAME_INFO_DT, FRAME_LAST, LIB_PATH,
                   LONG_GAPLESS, MP3D_FEAT_LOG10, OPT_CRC_CHECK, PACK_FLUSH, PACK_GAPLESS, PITCH_FRAME_DT, RATES,
                   WINDOW_NO_END,
                   FrameInfo, MP3DError, StreamInfo, _bind, _check, _load, _loaded, _pack_flags, _ptr, _stream, lib,
                   library)


def _host(x, dtype):
    """x as it is when None or a device tensor, else a C-contiguous host array of dtype"""
    return x if x is None or hasattr(x, "data_ptr") else np.ascontiguousarray(x, dtype)


class Decoder:
    """Per-frame decoder (mp3d_decode_frame), one per stream."""

    _h = None  # (no handle yet: close() after a failed create has nothing to destroy)

    def __init__(self, device=None):
        L = self._L = lib()  # the build that owns the handle: every later call goes to it
        h = ctypes.c_void_p()
        if device is None:
            _check(L.mp3d_dec_create(ctypes.byref(h)), L)
        else:
            _check(L.mp3d_dec_create_on(int(device), ctypes.byref(h)), L)
        self._h = h

    def _ck(self, rc):
        return _check(rc, self._L)

    def close(self):
        if self._h:
            self._L.mp3d_dec_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        self._L.mp3d_dec_reset(self._h)

    def set_options(self, flags):
        """MP3D_OPT_* flags (OPT_CRC_CHECK) for later decode calls."""
        self._ck(self._L.mp3d_dec_set_options(self._h, int(flags)))

    def decode_frame(self, buf, f32=False, last=False):
        """Returns (samples_per_channel, pcm [samples*channels], FrameInfo);
        pcm is int16, or float32 (full scale 1.0, unclipped) with f32=True.
        last=True: buf holds the rest of the stream, so a final frame cut
        short decodes with its missing bytes as zeros (MP3D_FRAME_LAST)."""
        pcm = np.zeros(2304, np.float32 if f32 else np.int16)
        info = FrameInfo()
        buf = bytes(buf)
        flags = (FRAME_F32 if f32 else 0) | (FRAME_LAST if last else 0)
        n = self._ck(self._L.mp3d_decode_frame_ex(self._h, buf, len(buf), pcm.ctypes.data, flags, ctypes.byref(info)))
        return n, pcm[: n * max(info.channels, 1)], info

    def get_state(self):
        """Opaque decoder state (np.uint8 [state_bytes()]) for set_state."""
        buf = np.zeros(state_bytes(), np.uint8)
        self._ck(self._L.mp3d_dec_get_state(self._h, buf.ctypes.data))
        return buf

    def set_state(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        if buf.size != state_bytes():
            raise ValueError("state blob of %d bytes, expected %d" % (buf.size, state_bytes()))
        self._ck(self._L.mp3d_dec_set_state(self._h, buf.ctypes.data))

    def stream_info(self):
        """StreamInfo of the stream decoded so far (Xing/Info tag, gapless)."""
        info = StreamInfo()
        self._ck(self._L.mp3d_dec_stream_info(self._h, ctypes.byref(info)))
        return info

    def decode_stream(self, data, gapless=False, f32=False):
        """Decode a whole byte stream; returns int16 (float32 with f32=True)
        [channels, samples].  gapless=True drops encoder delay / padding as
        the stream's LAME tag says (gapless_trim)."""
        if gapless:
            return gapless_trim(self.decode_stream(data, f32=f32), self.stream_info())
        data = bytes(data)
        pos, out, nch = 0, [], 0
        while pos < len(data):
            try:
                n, pcm, info = self.decode_frame(data[pos:], f32=f32, last=True)
            except MP3DError:
                break
            if info.frame_bytes <= 0:
                break
            pos += info.frame_bytes
            if n:
                nch = info.channels
                out.append(pcm.reshape(n, nch))
        if not out:
            return np.zeros((0, 0), np.float32 if f32 else np.int16)
        return np.concatenate(out).T.copy()


class BatchDecoder:
    """Batched decoder: per-stream state stays in HBM across calls."""

    _h = None  # (no handle yet: close() after a failed create has nothing to destroy)
    # What the wrapper knows of the handle's sinks, as the handle starts out.
    _out = (0, 0)  # the packed format (hz, channels); hz = 0: off
    _mels = 0  # feature sink: its number of mel filters
    _loud = False  # loudness sink
    _tp = False  # true-peak tap
    _stretch = False  # tempo sink
    _limit = None  # limiter: its ceiling in dBTP while it is on
    _segments = None  # segment sink: its pause and shortest segment in hops while it is on
    _eq = 0  # equaliser: its number of bands
    _pitch = None  # pitch sink: its lowest frequency in Hz while it is on
    _AFTER_PACKED = ("_mels", "_loud", "_tp", "_stretch", "_limit", "_segments", "_eq", "_pitch")

    def __init__(self, max_streams, max_frames, device=0):
        L = self._L = lib()  # the build that owns the handle: every later call goes to it
        h = ctypes.c_void_p()
        _check(L.mp3d_batch_create(int(device), int(max_streams), int(max_frames), ctypes.byref(h)), L)
        self._h = h
        self.device = device
        self.max_streams, self.max_frames = max_streams, max_frames

    def _ck(self, rc):
        return _check(rc, self._L)

    def _stage_us(self, fn):
        t = ctypes.c_float()
        self._ck(fn(self._h, ctypes.byref(t)))
        return float(t.value)

    def close(self):
        if self._h:
            self._L.mp3d_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        self._ck(self._L.mp3d_batch_reset(self._h))

    def set_options(self, flags):
        """MP3D_OPT_* flags (OPT_CRC_CHECK) for later decode calls."""
        self._ck(self._L.mp3d_batch_set_options(self._h, int(flags)))

    def sync(self):
        self._ck(self._L.mp3d_batch_sync(self._h))

    def set_timing(self, on=True):
        self._ck(self._L.mp3d_batch_set_timing(self._h, int(on)))

    def kernel_times_us(self):
        t = np.zeros(3, np.float32)
        self._ck(self._L.mp3d_batch_kernel_times(self._h, t.ctypes.data))
        return dict(zip(("demux", "huffman", "synth"), t.tolist()))

    @staticmethod
    def _geom(offsets, sizes):
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        sz = np.ascontiguousarray(sizes, dtype=np.uint32)
        if off.shape != sz.shape:
            raise ValueError("offsets/sizes shape mismatch")
        return off, sz

    def _decode_head(self, frames, offsets, sizes, frames_per_stream, infos=None):
        """The start of every decode call: (head, n, F, infos, keep) with head
        the leading C arguments (handle, frames, offsets, sizes, n_streams,
        frames_per_stream), infos the caller's or a host array [n, F], and
        keep what head points into, to hold until the call has returned."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, keep = _ptr(frames)
        return (self._h, fp, off.ctypes.data, sz.ctypes.data, n, F), n, F, infos, (keep, off, sz)

    @staticmethod
    def _stage_head(samples, counts, stride=None):
        """The start of every stage-alone call: (head, n, ss, keep) with head
        the C arguments after the handle (samples or NULL when there are none,
        sample_stride, counts, n_streams); samples [n, ss, ...], ss read from
        stride when given; counts int32 [n], a host sequence or a device
        tensor; keep as in _decode_head."""
        n, ss = int(samples.shape[0]), int(samples.shape[1]) if stride is None else int(stride)
        counts = _host(counts, np.int32)
        sp, cp = _ptr(samples)[0], _ptr(counts)[0]
        return (sp if ss else None, ss, cp, n), n, ss, counts

    @staticmethod
    def _sink_out(n, out, counts, stride, on, bound, tail, dtype):
        """The output of every sink call: (out, counts, stride).  The stride
        is out's, else bound() if the sink is on, else 1 (the call then fails
        with MP3D_E_ARG); out [n, stride, *tail] of dtype and counts int32 [n]
        are host arrays unless given."""
        if stride is None:
            stride = int(out.shape[1]) if out is not None else bound() if on else 1
        stride = int(stride)
        if out is None:
            out = np.zeros((n, stride) + tuple(tail), dtype)
        if counts is None:
            counts = np.zeros(n, np.int32)
        return out, counts, stride

    def decode(self, frames, offsets, sizes, frames_per_stream, pcm=None, infos=None, stream=None, f32=False):
        """frames: bytes/np.uint8/torch.uint8; pcm: None (allocate host) or
        int16 (float32 with f32=True) array/tensor [n, F, 2304]; infos: None
        or FRAME_INFO_DT array / int32 tensor [n, F, 6].  Returns (pcm, infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        if pcm is None:
            pcm = np.zeros((n, F, 2304), np.float32 if f32 else np.int16)
        fn = self._L.mp3d_batch_decode_f32 if f32 else self._L.mp3d_batch_decode
        self._ck(fn(*head, _ptr(pcm)[0], _ptr(infos)[0], _stream(stream)))
        return pcm, infos

    def set_output(self, hz, channels):
        """Format of the packed sink (decode_packed): hz from RATES, channels
        1 or 2; hz = 0 turns the sink off and frees its buffers.  A change
        restarts every stream's resampler."""
        self._ck(self._L.mp3d_batch_set_output(self._h, int(hz), int(channels)))
        self._out = (int(hz), int(channels))
        for name in self._AFTER_PACKED:  # a change of the output format turns every sink after the packed one off
            setattr(self, name, getattr(BatchDecoder, name))

    def decode_packed(self, frames, offsets, sizes, frames_per_stream, out=None, counts=None, infos=None, f32=True,
                      flush=False, stride=None, stream=None, gapless=False):
        """Decode and write every stream's samples contiguously at the rate
        and channel count of set_output (mp3d_batch_decode_packed).  out: None
        (allocate host) or float32 (int16 with f32=False) array/tensor
        [n, stride, channels]; counts: None or int32 array/tensor [n]; infos as
        in decode.  stride defaults to out's, else to the bound that cannot
        overflow.  flush=True ends the streams: the filter tails are emitted
        and the resamplers restart.  gapless=True fixes the sample window of
        every stream that has none yet from its LAME tag (set_window).  Returns
        (out, counts, infos); stream s holds counts[s] samples per channel
        (-1: over the stride)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        hz, ch = self._out
        out, counts, stride = self._sink_out(n, out, counts, stride, hz, lambda: packed_max_samples(hz, F), (ch,),
                                             np.float32 if f32 else np.int16)
        self._ck(self._L.mp3d_batch_decode_packed(*head, _ptr(out)[0], int(bool(f32)), stride, _ptr(counts)[0],
                                                  _pack_flags(flush, gapless), _ptr(infos)[0], _stream(stream)))
        return out, counts, infos

    def set_window(self, lo, hi=None, first=0):
        """Fix the sample windows [lo[i], hi[i]) of streams first, first + 1 ...
        (mp3d_batch_set_window), in input samples per channel counted from the
        next sample fed: only those reach the packed and the feature sink.  hi:
        None (no end for all) or a sequence whose None / WINDOW_NO_END elements
        mean no end.  lo=None clears the windows of every stream from first on.
        The streams' resamplers and feature state restart."""
        first = int(first)
        if lo is None:
            if hi is not None:
                raise ValueError("hi without lo")
            n = self.max_streams - first
            self._ck(self._L.mp3d_batch_set_window(self._h, first, n, None, None))
            return
        lo = np.ascontiguousarray(lo, np.int64).reshape(-1)
        n = lo.size
        hp = None
        if hi is not None:
            hi = np.array([WINDOW_NO_END if h is None else int(h) for h in hi], np.int64)
            if hi.size != n:
                raise ValueError("lo / hi length mismatch")
            if (hi < lo).any():
                raise ValueError("window with hi < lo")
            hp = hi.ctypes.data
        if (lo < 0).any():
            raise ValueError("window with lo < 0")
        self._ck(self._L.mp3d_batch_set_window(self._h, first, n, lo.ctypes.data, hp))

    def sink_window(self, first=0, n=None):
        """(lo, hi, fed) of streams [first, first + n): int64 arrays, the
        sample windows and the samples fed since the last window restart
        (mp3d_batch_sink_window).  A stream without a fixed window reports
        (0, WINDOW_NO_END, 0)."""
        first = int(first)
        n = self.max_streams - first if n is None else int(n)
        lo, hi, fed = (np.zeros(max(n, 0), np.int64) for _ in range(3))
        self._ck(self._L.mp3d_batch_sink_window(self._h, first, n, lo.ctypes.data, hi.ctypes.data, fed.ctypes.data))
        return lo, hi, fed

    def resample_time_us(self):
        """Device-side microseconds of the resample stage of the last packed
        call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_resample_time)

    def set_features(self, n_mels, log10=True):
        """Turn the log-mel feature sink on (mp3d_batch_set_features): n_mels
        Slaney filters (1 .. 128) over 25 ms Hann frames every 10 ms of the
        16 kHz mono packed output, log10(max(mel, 1e-10)) or, with
        log10=False, the mel energies.  Needs set_output(16000, 1).  n_mels = 0
        turns it off.  Restarts every stream's feature state."""
        self._ck(self._L.mp3d_batch_set_features(self._h, int(n_mels), FEAT_LOG10 if log10 else 0))
        self._mels = int(n_mels)

    def decode_features(self, frames, offsets, sizes, frames_per_stream, feat=None, counts=None, infos=None,
                        flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does and write every stream's log-mel
        frames (mp3d_batch_decode_features).  feat: None (allocate host) or
        float32 array/tensor [n, stride, n_mels]; counts: None or int32
        array/tensor [n]; infos as in decode.  stride defaults to feat's, else
        to feat_max_frames.  flush=True ends the streams: resampler and
        feature tails are emitted and both restart.  gapless as in
        decode_packed.  Returns (feat, counts, infos); stream s holds
        counts[s] frames (-1: over the stride)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        feat, counts, stride = self._sink_out(n, feat, counts, stride, self._mels, lambda: feat_max_frames(F),
                                              (max(self._mels, 1),), np.float32)
        self._ck(self._L.mp3d_batch_decode_features(*head, _ptr(feat)[0], stride, _ptr(counts)[0],
                                                    _pack_flags(flush, gapless), _ptr(infos)[0], _stream(stream)))
        return feat, counts, infos

    def features(self, samples, counts, feat=None, feat_counts=None, flush=False, stride=None, stream=None):
        """The feature stage alone (mp3d_batch_features): samples float32
        [n, sample_stride] 16 kHz mono, counts int32 [n] samples per stream
        (both host arrays or device tensors), through the same kernels and
        per-stream state as decode_features.  Returns (feat, feat_counts)."""
        head, n, ss, keep = self._stage_head(samples, counts)
        feat, feat_counts, stride = self._sink_out(n, feat, feat_counts, stride, self._mels,
                                                   lambda: (ss + 200 + 159) // 160 + 1, (max(self._mels, 1),),
                                                   np.float32)
        self._ck(self._L.mp3d_batch_features(self._h, *head, _ptr(feat)[0], stride, _ptr(feat_counts)[0],
                                             _pack_flags(flush), _stream(stream)))
        return feat, feat_counts

    def feature_time_us(self):
        """Device-side microseconds of the feature stage of the last feature
        call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_feature_time)

    def set_loudness(self, on=True):
        """Turn the loudness sink on or off (mp3d_batch_set_loudness): ITU-R
        BS.1770-4 K-weighted 100 ms block energies and the sample peak of the
        packed output, whatever its format.  Needs set_output.  Restarts every
        stream's loudness state."""
        self._ck(self._L.mp3d_batch_set_loudness(self._h, int(bool(on))))
        self._loud = bool(on)

    def loudness(self, samples, counts, blocks=None, block_counts=None, peak=None, flush=False, stride=None,
                 stream=None):
        """The loudness stage alone (mp3d_batch_loudness): samples float32
        [n, sample_stride, channels] in the packed format, counts int32 [n]
        sample frames per stream (both host arrays or device tensors), e.g.
        the device out and counts of decode_packed.  blocks: None (allocate
        host) or float32 array/tensor [n, stride]; block_counts int32 [n]; peak
        float32 [n].  flush=True drops the open block and restarts the streams.
        Returns (blocks, block_counts, peak): stream s holds block_counts[s]
        block energies (-1: over the stride)."""
        head, n, ss, keep = self._stage_head(samples, counts)
        H = (self._out[0] + 5) // 10
        blocks, block_counts, stride = self._sink_out(n, blocks, block_counts, stride, self._loud,
                                                      lambda: (H - 1 + ss) // H, (), np.float32)
        peak = np.zeros(n, np.float32) if peak is None else peak
        self._ck(self._L.mp3d_batch_loudness(self._h, *head, _ptr(blocks)[0], stride, _ptr(block_counts)[0],
                                             _ptr(peak)[0], _pack_flags(flush), _stream(stream)))
        return blocks, block_counts, peak

    def decode_loudness(self, frames, offsets, sizes, frames_per_stream, blocks=None, counts=None, peak=None,
                        infos=None, flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does and write every stream's block
        energies and sample peak (mp3d_batch_decode_loudness).  stride
        defaults to blocks', else to loud_max_blocks.  flush and gapless as in
        decode_packed; the flush also drops the open block.  Returns (blocks,
        counts, peak, infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        blocks, counts, stride = self._sink_out(n, blocks, counts, stride, self._loud,
                                                lambda: loud_max_blocks(self._out[0], F), (), np.float32)
        peak = np.zeros(n, np.float32) if peak is None else peak
        self._ck(self._L.mp3d_batch_decode_loudness(*head, _ptr(blocks)[0], stride, _ptr(counts)[0], _ptr(peak)[0],
                                                    _pack_flags(flush, gapless), _ptr(infos)[0], _stream(stream)))
        return blocks, counts, peak, infos

    def integrated_lufs(self, blocks, counts, lufs=None, stream=None):
        """Gated integrated loudness of every row of blocks float32
        [n, stride] holding counts[s] block energies, on the GPU
        (mp3d_batch_loudness_integrated); host arrays or device tensors.
        Returns lufs float32 [n], -inf for a row of fewer than 4 blocks."""
        head, n, stride, keep = self._stage_head(blocks, counts)
        if lufs is None:
            lufs = np.zeros(n, np.float32)
        self._ck(self._L.mp3d_batch_loudness_integrated(self._h, *head, _ptr(lufs)[0], _stream(stream)))
        return lufs

    def loudness_time_us(self):
        """Device-side microseconds of the loudness stage of the last
        loudness call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_loudness_time)

    def set_true_peak(self, on=True):
        """Turn the true-peak tap on or off (mp3d_batch_set_true_peak): the
        4x oversampled peak of the packed output, whatever its format.  Needs
        set_output.  Restarts every stream's true-peak state."""
        self._ck(self._L.mp3d_batch_set_true_peak(self._h, int(bool(on))))
        self._tp = bool(on)

    def true_peak(self, samples, counts, tpeak=None, flush=False, stride=None, stream=None):
        """The true-peak tap (mp3d_batch_true_peak): samples float32
        [n, sample_stride, channels] in the packed format, counts int32 [n]
        sample frames per stream (both host arrays or device tensors), e.g.
        the device out and counts of decode_packed; stride: the sample stride
        when it is not samples.shape[1].  tpeak: None (allocate host) or
        float32 array/tensor [n].  flush=True emits the last 6 indices of every
        stream and restarts it.  Returns tpeak; the true peak of a stream fed
        in several calls is the max of theirs."""
        head, n, ss, keep = self._stage_head(samples, counts, stride)
        if tpeak is None:
            tpeak = np.zeros(n, np.float32)
        self._ck(self._L.mp3d_batch_true_peak(self._h, *head, _ptr(tpeak)[0], _pack_flags(flush), _stream(stream)))
        return tpeak

    def decode_measure(self, frames, offsets, sizes, frames_per_stream, blocks=None, counts=None, peak=None,
                       tpeak=None, infos=None, flush=False, stride=None, stream=None, gapless=False):
        """decode_loudness plus the true-peak tap on the same samples
        (mp3d_batch_decode_measure); needs set_loudness and set_true_peak.
        Returns (blocks, counts, peak, tpeak, infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        blocks, counts, stride = self._sink_out(n, blocks, counts, stride, self._loud,
                                                lambda: loud_max_blocks(self._out[0], F), (), np.float32)
        peak = np.zeros(n, np.float32) if peak is None else peak
        tpeak = np.zeros(n, np.float32) if tpeak is None else tpeak
        self._ck(self._L.mp3d_batch_decode_measure(*head, _ptr(blocks)[0], stride, _ptr(counts)[0], _ptr(peak)[0],
                                                   _ptr(tpeak)[0], _pack_flags(flush, gapless), _ptr(infos)[0],
                                                   _stream(stream)))
        return blocks, counts, peak, tpeak, infos

    def normalize_gain(self, lufs, tpeak=None, target=-23.0, max_dbtp=-1.0, gain=None, stream=None):
        """The gain that brings each stream from lufs[s] to target LUFS,
        limited so that gain * tpeak[s] stays at or below max_dbtp dBTP
        (mp3d_batch_normalize_gain); tpeak=None: no limit.  A stream whose
        loudness is not finite gets gain 1.  Host arrays or device tensors,
        float32 [n].  Returns gain."""
        lufs, tpeak = _host(lufs, np.float32), _host(tpeak, np.float32)
        n = int(lufs.shape[0])
        if gain is None:
            gain = np.zeros(n, np.float32)
        self._ck(self._L.mp3d_batch_normalize_gain(self._h, _ptr(lufs)[0], _ptr(tpeak)[0], n, float(target),
                                                   float(max_dbtp), _ptr(gain)[0], _stream(stream)))
        return gain

    def apply_gain(self, samples, counts, gain, out=None, f32=True, stream=None):
        """out[s, i, c] = samples[s, i, c] * gain[s] for i < counts[s]
        (mp3d_batch_apply_gain): samples float32 [n, stride, channels] in the
        packed format, counts int32 [n], gain float32 [n]; out: None (allocate
        host, zeros past the counts) or float32 (int16 with f32=False)
        array/tensor of samples' shape, which may be samples itself for
        float32.  Nothing past counts[s] is written.  Returns out."""
        head, n, ss, keep = self._stage_head(samples, counts)
        gain = _host(gain, np.float32)
        if out is None:
            out = np.zeros(tuple(samples.shape), np.float32 if f32 else np.int16)
        self._ck(self._L.mp3d_batch_apply_gain(self._h, *head, _ptr(gain)[0], _ptr(out)[0], int(bool(f32)),
                                               _stream(stream)))
        return out

    def true_peak_time_us(self):
        """Device-side microseconds of the true-peak stage of the last
        true-peak call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_true_peak_time)

    def set_stretch(self, on=True):
        """Turn the tempo sink on or off (mp3d_batch_set_stretch): a
        pitch-preserving time stretch of the packed output, whatever its
        format.  Needs set_output.  Restarts every stream's stretch state and
        sets every stream's tempo to 1/1."""
        self._ck(self._L.mp3d_batch_set_stretch(self._h, int(bool(on))))
        self._stretch = bool(on)

    def set_tempo(self, num, den, first=0):
        """The tempo num / den of streams first, first + 1 ...
        (mp3d_batch_set_tempo): integers in [1, 4096] with 1/2 <= num/den <= 2,
        scalars (one stream) or equally long sequences.  The output plays
        num/den times as fast.  Restarts those streams' stretch state."""
        num = np.ascontiguousarray(num, np.int32).reshape(-1)
        den = np.ascontiguousarray(den, np.int32).reshape(-1)
        if num.size != den.size:
            raise ValueError("num / den length mismatch")
        self._ck(self._L.mp3d_batch_set_tempo(self._h, int(first), num.size, num.ctypes.data, den.ctypes.data))

    def stretch(self, samples, counts, out=None, out_counts=None, flush=False, stride=None, stream=None):
        """The tempo sink alone (mp3d_batch_stretch): samples float32
        [n, sample_stride, channels] in the packed format, counts int32 [n]
        sample frames per stream (both host arrays or device tensors), e.g.
        the device out and counts of decode_packed.  out: None (allocate host)
        or float32 array/tensor [n, stride, channels], not overlapping samples;
        out_counts int32 [n].  stride defaults to out's, else to the bound
        that cannot overflow at the slowest tempo.  flush=True emits the rest
        of every stream and restarts it.  Returns (out, out_counts): stream s
        holds out_counts[s] samples per channel (-1: over the stride)."""
        head, n, ss, keep = self._stage_head(samples, counts)
        hz, ch = self._out
        out, out_counts, stride = self._sink_out(n, out, out_counts, stride, self._stretch,
                                                 lambda: stretch_max_samples(hz, ss, 1, 2), (ch,), np.float32)
        self._ck(self._L.mp3d_batch_stretch(self._h, *head, _ptr(out)[0], stride, _ptr(out_counts)[0],
                                            _pack_flags(flush), _stream(stream)))
        return out, out_counts

    def decode_stretched(self, frames, offsets, sizes, frames_per_stream, out=None, counts=None, infos=None,
                         flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        samples at its tempo (mp3d_batch_decode_stretched).  stride defaults to
        out's, else to the bound that cannot overflow at the slowest tempo.
        flush and gapless as in decode_packed; the flush also ends the
        stretch.  Returns (out, counts, infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        hz, ch = self._out
        out, counts, stride = self._sink_out(
            n, out, counts, stride, self._stretch, lambda: stretch_max_samples(hz, packed_max_samples(hz, F), 1, 2),
            (ch,), np.float32)
        self._ck(self._L.mp3d_batch_decode_stretched(*head, _ptr(out)[0], stride, _ptr(counts)[0],
                                                     _pack_flags(flush, gapless), _ptr(infos)[0], _stream(stream)))
        return out, counts, infos

    def stretch_time_us(self):
        """Device-side microseconds of the stretch stage of the last stretch
        call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_stretch_time)

    def set_limiter(self, on=True, ceiling_db=-1.0):
        """Turn the look-ahead true-peak limiter on or off
        (mp3d_batch_set_limiter): a per-sample gain on the packed output,
        whatever its format, that holds the 4x oversampled peak of every sample
        frame at or below ceiling_db dBTP (-20 .. 0).  Needs set_output.
        Restarts every stream's limiter state."""
        self._ck(self._L.mp3d_batch_set_limiter(self._h, int(bool(on)), float(ceiling_db)))
        self._limit = float(ceiling_db) if on else None

    def limit(self, samples, counts, gain=None, out=None, out_counts=None, gr=None, f32=True, flush=False, stride=None,
              stream=None):
        """The limiter alone (mp3d_batch_limit): samples float32
        [n, sample_stride, channels] in the packed format, counts int32 [n]
        sample frames per stream (both host arrays or device tensors), e.g.
        the device out and counts of decode_packed; gain float32 [n], applied
        before the limiter (None: 1).  out: None (allocate host) or float32
        (int16 with f32=False) array/tensor [n, stride, channels], not
        overlapping samples; out_counts int32 [n]; gr float32 [n] receives the
        smallest gain of the call per stream.  stride defaults to out's, else
        to the bound that cannot overflow.  flush=True emits the last A + 6
        samples of every stream and restarts it.  Returns (out, out_counts,
        gr): stream s holds out_counts[s] samples per channel (-1: over the
        stride)."""
        head, n, ss, keep = self._stage_head(samples, counts)
        hz, ch = self._out
        out, out_counts, stride = self._sink_out(n, out, out_counts, stride, self._limit is not None,
                                                 lambda: limiter_max_samples(hz, ss), (ch,),
                                                 np.float32 if f32 else np.int16)
        gain = _host(gain, np.float32)
        gr = np.ones(n, np.float32) if gr is None else gr
        self._ck(self._L.mp3d_batch_limit(self._h, *head, _ptr(gain)[0], _ptr(out)[0], int(bool(f32)), stride,
                                          _ptr(out_counts)[0], _ptr(gr)[0], _pack_flags(flush), _stream(stream)))
        return out, out_counts, gr

    def decode_limited(self, frames, offsets, sizes, frames_per_stream, gain=None, out=None, counts=None, gr=None,
                       infos=None, f32=True, flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        samples times gain through the limiter (mp3d_batch_decode_limited).
        stride defaults to out's, else to the bound that cannot overflow.
        flush and gapless as in decode_packed; the flush also ends the
        limiter.  Returns (out, counts, gr, infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        hz, ch = self._out
        out, counts, stride = self._sink_out(
            n, out, counts, stride, self._limit is not None, lambda: limiter_max_samples(hz, packed_max_samples(hz, F)),
            (ch,), np.float32 if f32 else np.int16)
        gain = _host(gain, np.float32)
        gr = np.ones(n, np.float32) if gr is None else gr
        self._ck(self._L.mp3d_batch_decode_limited(*head, _ptr(gain)[0], _ptr(out)[0], int(bool(f32)), stride,
                                                   _ptr(counts)[0], _ptr(gr)[0], _pack_flags(flush, gapless),
                                                   _ptr(infos)[0], _stream(stream)))
        return out, counts, gr, infos

    def limiter_time_us(self):
        """Device-side microseconds of the limiter stage of the last limiter
        call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_limiter_time)

    def set_eq(self, bands, preamp_db=0.0):
        """Set the equaliser's curve (mp3d_batch_set_eq): bands a list of up
        to EQ_MAX_BANDS (type, f0_hz, gain_db, q) with type one of EQ_PEAK,
        EQ_LOW_SHELF, EQ_HIGH_SHELF, EQ_HIGH_PASS, EQ_LOW_PASS, applied in
        order to every channel of the packed output; preamp_db scales the
        whole curve.  None or [] turns the equaliser off.  Needs set_output.
        Restarts every stream's equaliser state."""
        arr = _eq_bands(bands)
        self._ck(self._L.mp3d_batch_set_eq(self._h, arr.ctypes.data if arr.size else None, arr.size,
                                           float(preamp_db)))
        self._eq = int(arr.size)

    def eq(self, samples, counts, out=None, out_counts=None, flush=False, stride=None, stream=None):
        """The equaliser alone (mp3d_batch_eq): samples float32
        [n, sample_stride, channels] in the packed format, counts int32 [n]
        sample frames per stream (both host arrays or device tensors), e.g.
        the device out and counts of decode_packed.  out: None (allocate host)
        or float32 array/tensor [n, stride, channels], not overlapping
        samples; out_counts int32 [n].  stride defaults to out's, else to
        sample_stride: the stage emits as many samples as it is fed.
        flush=True restarts the streams after the call.  Returns (out,
        out_counts): stream s holds out_counts[s] samples per channel (-1:
        over the stride)."""
        head, n, ss, keep = self._stage_head(samples, counts)
        out, out_counts, stride = self._sink_out(n, out, out_counts, stride, self._eq, lambda: ss, (self._out[1],),
                                                 np.float32)
        self._ck(self._L.mp3d_batch_eq(self._h, *head, _ptr(out)[0], stride, _ptr(out_counts)[0], _pack_flags(flush),
                                       _stream(stream)))
        return out, out_counts

    def decode_equalized(self, frames, offsets, sizes, frames_per_stream, out=None, counts=None, infos=None,
                         flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        samples through the equaliser (mp3d_batch_decode_equalized).  stride
        defaults to out's, else to the bound that cannot overflow.  flush and
        gapless as in decode_packed; the flush also restarts the equaliser.
        Returns (out, counts, infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        hz, ch = self._out
        out, counts, stride = self._sink_out(n, out, counts, stride, self._eq, lambda: packed_max_samples(hz, F), (ch,),
                                             np.float32)
        self._ck(self._L.mp3d_batch_decode_equalized(*head, _ptr(out)[0], stride, _ptr(counts)[0],
                                                     _pack_flags(flush, gapless), _ptr(infos)[0], _stream(stream)))
        return out, counts, infos

    def eq_time_us(self):
        """Device-side microseconds of the equaliser stage of the last
        equaliser call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_eq_time)

    def set_segments(self, on=True, threshold_db=-40.0, min_pause_ms=300, min_speech_ms=100, pad_ms=50):
        """Turn the segment sink on or off (mp3d_batch_set_segments): the
        sample ranges of the packed output, whatever its format, in which the
        energy of 10 ms hops stays at or over threshold_db dBFS (-96 .. 0),
        pauses shorter than min_pause_ms filled, then runs shorter than
        min_speech_ms dropped, each range widened by pad_ms (at most half the
        pause).  The times become hops by round(ms / 10); the defaults are
        conventions, not measurements.  Needs set_output.  Restarts every
        stream's segment state."""
        hops = [int(round(ms / 10.0)) for ms in (min_pause_ms, min_speech_ms, pad_ms)]
        self._ck(self._L.mp3d_batch_set_segments(self._h, int(bool(on)), *hops))
        self._segments = (hops[0], hops[1]) if on else None
        if on and float(threshold_db) != -40.0:
            self.set_segment_threshold(db=threshold_db, n=self.max_streams)

    def set_segment_threshold(self, db=None, energy=None, first=0, n=1):
        """The threshold of streams first, first + 1 ...
        (mp3d_batch_set_segment_threshold): energy, hop energies in
        [1, H * 2^30] (a scalar or a sequence, one per stream), or db, one
        level in dBFS for n streams (segment_threshold).  Restarts those
        streams' segment state."""
        if (db is None) == (energy is None):
            raise ValueError("one of db and energy")
        if energy is None:
            energy = [segment_threshold(self._out[0], db)] * int(n)
        thr = np.ascontiguousarray(energy, np.uint64).reshape(-1)
        self._ck(self._L.mp3d_batch_set_segment_threshold(self._h, int(first), thr.size, thr.ctypes.data))

    def segments(self, samples, counts, seg=None, seg_counts=None, flush=False, stride=None, stream=None):
        """The segment sink alone (mp3d_batch_segments): samples float32
        [n, sample_stride, channels] in the packed format, counts int32 [n]
        sample frames per stream (both host arrays or device tensors), e.g.
        the device out and counts of decode_packed, stretch or limit.  seg:
        None (allocate host) or int64 array/tensor [n, stride, 2]; seg_counts
        int32 [n].  stride defaults to seg's, else to the bound that cannot
        overflow.  flush=True emits the rest of every stream, an open segment
        closed at its end, and restarts it.  Returns (seg, seg_counts): stream
        s holds seg_counts[s] pairs (start, end) in samples since its restart
        (-1: over the stride)."""
        head, n, ss, keep = self._stage_head(samples, counts)
        seg, seg_counts, stride = self._sink_out(n, seg, seg_counts, stride, self._segments is not None,
                                                 lambda: segment_max(self._out[0], ss, *self._segments), (2,), np.int64)
        self._ck(self._L.mp3d_batch_segments(self._h, *head, _ptr(seg)[0], stride, _ptr(seg_counts)[0],
                                             _pack_flags(flush), _stream(stream)))
        return seg, seg_counts

    def decode_segments(self, frames, offsets, sizes, frames_per_stream, seg=None, counts=None, infos=None,
                        flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        segments (mp3d_batch_decode_segments).  stride defaults to seg's, else
        to the bound that cannot overflow.  flush and gapless as in
        decode_packed; the flush also ends the segments.  Returns (seg, counts,
        infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        hz = self._out[0]
        seg, counts, stride = self._sink_out(
            n, seg, counts, stride, self._segments is not None,
            lambda: segment_max(hz, packed_max_samples(hz, F), *self._segments), (2,), np.int64)
        self._ck(self._L.mp3d_batch_decode_segments(*head, _ptr(seg)[0], stride, _ptr(counts)[0],
                                                    _pack_flags(flush, gapless), _ptr(infos)[0], _stream(stream)))
        return seg, counts, infos

    def segment_time_us(self):
        """Device-side microseconds of the segment stage of the last segment
        call (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_segment_time)

    def long_segments(self, data, segment_frames=32, gapless=True):
        """The sentences of one file: decode_long_packed at the handle's
        format into a tensor on the handle's device, then segments(flush=True)
        on it as one stream.  Needs set_segments.  Returns (int64 [k, 2] of
        (start, end) in samples, the pcm tensor [n, channels], StreamInfo,
        in_hz)."""
        import torch

        hz, ch = self._out
        if self._segments is None:
            raise MP3DError("long_segments needs set_segments")
        host = data.cpu().numpy().tobytes() if hasattr(data, "cpu") else bytes(data)
        cap = max(1, long_packed_bound(host, hz))
        out = torch.zeros((cap, ch), dtype=torch.float32, device="cuda:%d" % self.device)
        pcm, si, in_hz = self.decode_long_packed(data, hz, ch, segment_frames, out=out, gapless=gapless)
        n = int(pcm.shape[0])
        seg, cnt = self.segments(out[None, : max(n, 1)], [n], flush=True)
        return seg[0, : int(cnt[0])].copy(), pcm, si, in_hz

    def set_pitch(self, on=True, fmin=60, fmax=500, threshold=0.15):
        """Turn the pitch sink on or off (mp3d_batch_set_pitch): one record
        (f0_hz, periodicity, lag, shift) per 10 ms of the packed output,
        whatever its format, by YIN over the lags of fmax .. fmin Hz (integers,
        50 <= fmin < fmax <= 2000, 4 fmax <= hz); a frame is voiced when its
        normalised difference falls under threshold, passed on as
        round(1024 * threshold) in 1 .. 1024.  Needs set_output.  Restarts
        every stream's pitch state."""
        theta = int(round(1024 * float(threshold)))
        self._ck(self._L.mp3d_batch_set_pitch(self._h, int(bool(on)), int(fmin), int(fmax), theta))
        self._pitch = int(fmin) if on else None

    def pitch(self, samples, counts, out=None, out_counts=None, flush=False, stride=None, stream=None):
        """The pitch sink alone (mp3d_batch_pitch): samples float32
        [n, sample_stride, channels] in the packed format, counts int32 [n]
        sample frames per stream (both host arrays or device tensors), e.g.
        the device out and counts of decode_packed, stretch, limit or eq.  out:
        None (allocate host) or a PITCH_FRAME_DT array [n, stride] (a device
        tensor: 16 bytes per record, e.g. int32 [n, stride, 4]); out_counts
        int32 [n].  stride defaults to out's, else to pitch_max_frames.
        flush=True emits every frame that starts inside the stream, zeros
        behind its end, and restarts it.  Returns (out, out_counts): stream s
        holds out_counts[s] records (-1: over the stride)."""
        head, n, ss, keep = self._stage_head(samples, counts)
        out, out_counts, stride = self._sink_out(n, out, out_counts, stride, self._pitch is not None,
                                                 lambda: pitch_max_frames(self._out[0], ss, self._pitch), (),
                                                 PITCH_FRAME_DT)
        self._ck(self._L.mp3d_batch_pitch(self._h, *head, _ptr(out)[0], stride, _ptr(out_counts)[0],
                                          _pack_flags(flush), _stream(stream)))
        return out, out_counts

    def decode_pitch(self, frames, offsets, sizes, frames_per_stream, out=None, counts=None, infos=None,
                     flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        pitch records (mp3d_batch_decode_pitch).  stride defaults to out's,
        else to the bound that cannot overflow.  flush and gapless as in
        decode_packed; the flush also ends the pitch frames.  Returns (out,
        counts, infos)."""
        head, n, F, infos, keep = self._decode_head(frames, offsets, sizes, frames_per_stream, infos)
        hz = self._out[0]
        out, counts, stride = self._sink_out(
            n, out, counts, stride, self._pitch is not None,
            lambda: pitch_max_frames(hz, packed_max_samples(hz, F), self._pitch), (), PITCH_FRAME_DT)
        self._ck(self._L.mp3d_batch_decode_pitch(*head, _ptr(out)[0], stride, _ptr(counts)[0],
                                                 _pack_flags(flush, gapless), _ptr(infos)[0], _stream(stream)))
        return out, counts, infos

    def pitch_time_us(self):
        """Device-side microseconds of the pitch stage of the last pitch call
        (after set_timing)."""
        return self._stage_us(self._L.mp3d_batch_pitch_time)

    def long_pitch(self, data, segment_frames=32, gapless=True):
        """The F0 contour of one file: decode_long_packed at the handle's
        format into a tensor on the handle's device, then pitch(flush=True) on
        it as one stream.  Needs set_pitch.  Returns (PITCH_FRAME_DT [k], the
        pcm tensor [n, channels], StreamInfo, in_hz)."""
        import torch

        hz, ch = self._out
        if self._pitch is None:
            raise MP3DError("long_pitch needs set_pitch")
        host = data.cpu().numpy().tobytes() if hasattr(data, "cpu") else bytes(data)
        cap = max(1, long_packed_bound(host, hz))
        out = torch.zeros((cap, ch), dtype=torch.float32, device="cuda:%d" % self.device)
        pcm, si, in_hz = self.decode_long_packed(data, hz, ch, segment_frames, out=out, gapless=gapless)
        n = int(pcm.shape[0])
        rec, cnt = self.pitch(out[None, : max(n, 1)], [n], flush=True)
        return rec[0, : int(cnt[0])].copy(), pcm, si, in_hz

    def decode_normalized(self, frames, offsets, sizes, frames_per_stream, target=-23.0, max_dbtp=-1.0, out=None,
                          f32=True, gapless=False, limit=False):
        """Decode streams that are whole in this call and normalise them to
        target LUFS under max_dbtp dBTP, all on the device with no host sync
        between the stages: decode_packed(flush), loudness(flush),
        true_peak(flush), integrated_lufs, normalize_gain, apply_gain.  Needs
        set_loudness and set_true_peak.  out: None (allocate host) or float32
        (int16 with f32=False) array/tensor [n, packed_max_samples, channels].
        limit=True (needs set_limiter with ceiling_db == max_dbtp): the gain
        is not capped by the true peak, so every stream reaches the target,
        and the limiter takes the place of apply_gain and holds the peaks
        under the ceiling; tpeak stays the measurement before it.
        Returns (out, counts, lufs, tpeak, gain, infos): out as given, the rest
        host arrays."""
        import torch
        if not (self._loud and self._tp):
            raise MP3DError("decode_normalized needs set_loudness and set_true_peak")
        if limit:
            if self._limit is None:
                raise MP3DError("decode_normalized(limit=True) needs set_limiter")
            if float(max_dbtp) != self._limit:
                raise MP3DError("max_dbtp %r is not the limiter's ceiling %r" % (max_dbtp, self._limit))
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        hz, ch = self._out
        S = packed_max_samples(hz, F)
        if out is None:
            out = np.zeros((n, S, ch), np.float32 if f32 else np.int16)
        if tuple(out.shape) != (n, S, ch):
            raise ValueError("out must be [%d, %d, %d]" % (n, S, ch))
        dev = torch.device("cuda", self.device)
        smp = torch.empty((n, S, ch), dtype=torch.float32, device=dev)
        counts, bc = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(2))
        nb = max((S + (hz + 5) // 10 - 1) // ((hz + 5) // 10), 1)
        blocks = torch.empty((n, nb), dtype=torch.float32, device=dev)
        peak, tpeak, lufs, gain = (torch.empty((n,), dtype=torch.float32, device=dev) for _ in range(4))
        infos = torch.empty((n, F, 6), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # (nothing of the allocator's is on the handle's stream)
        self.decode_packed(frames, off, sz, F, out=smp, counts=counts, infos=infos, flush=True, gapless=gapless)
        self.loudness(smp, counts, blocks=blocks, block_counts=bc, peak=peak, flush=True)
        self.true_peak(smp, counts, tpeak=tpeak, flush=True)
        self.integrated_lufs(blocks, bc, lufs=lufs)
        if limit:
            self.normalize_gain(lufs, None, target=target, max_dbtp=max_dbtp, gain=gain)
            oc, gr = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
            self.limit(smp, counts, gain, out=out, out_counts=oc, gr=gr, f32=f32, flush=True)
        else:
            self.normalize_gain(lufs, tpeak, target=target, max_dbtp=max_dbtp, gain=gain)
            self.apply_gain(smp, counts, gain, out=out, f32=f32)
        self.sync()
        infos = infos.cpu().numpy().view(FRAME_INFO_DT).reshape(n, F)
        return out, counts.cpu().numpy(), lufs.cpu().numpy(), tpeak.cpu().numpy(), gain.cpu().numpy(), infos

    @staticmethod
    def _nbytes(x):
        """Byte size of a contiguous host array / device tensor (its element
        count times element size, whatever the dtype)."""
        if hasattr(x, "numel"):
            if not x.is_contiguous():
                raise ValueError("state tensor must be contiguous")
            return x.numel() * x.element_size()
        if not isinstance(x, np.ndarray) or not x.flags.c_contiguous:
            raise ValueError("state buffer must be a C-contiguous numpy array or tensor")
        return x.nbytes

    def _state_range(self, first, n):
        first, n = int(first), int(n)
        if first < 0 or n <= 0 or first + n > self.max_streams:
            raise ValueError("streams [%d, %d) outside the handle's %d" % (first, first + n, self.max_streams))
        return first, n

    def get_state(self, first=0, n=None, out=None):
        """State blobs of streams [first, first + n): np.uint8 [n, state_bytes()]
        (or into `out`, a host array or device tensor of exactly that many
        bytes)."""
        first, n = self._state_range(first, self.max_streams - int(first) if n is None else n)
        if out is None:
            out = np.zeros((n, state_bytes()), np.uint8)
        if self._nbytes(out) != n * state_bytes():
            raise ValueError("out holds %d bytes, %d streams need %d" % (self._nbytes(out), n, n * state_bytes()))
        op, k = _ptr(out)
        self._ck(self._L.mp3d_batch_get_state(self._h, first, n, op))
        return out

    def set_state(self, buf, first=0):
        """Restore state blobs [n, state_bytes()] into streams [first, first + n);
        buf is a contiguous host array or device tensor of n * state_bytes()
        bytes (any dtype: the byte count decides n)."""
        if not hasattr(buf, "numel"):
            buf = np.asarray(buf)
            if not buf.flags.c_contiguous:
                raise ValueError("state buffer must be C-contiguous")
        nb = self._nbytes(buf)
        if nb == 0 or nb % state_bytes():
            raise ValueError("state buffer of %d bytes is not a whole number of %d-byte blobs" % (nb, state_bytes()))
        first, n = self._state_range(first, nb // state_bytes())
        bp, k = _ptr(buf)
        self._ck(self._L.mp3d_batch_set_state(self._h, first, n, bp))

    def stream_info(self, n_streams):
        """[StreamInfo] of the first n_streams streams (after a decode call)."""
        arr = (StreamInfo * int(n_streams))()
        self._ck(self._L.mp3d_batch_stream_info(self._h, int(n_streams), ctypes.cast(arr, ctypes.c_void_p)))
        return list(arr)

    def decode_long(self, data, segment_frames=32, max_frames=None, pcm=None, infos=None, f32=False):
        """Frame-parallel decode of ONE long stream (mp3d_batch_decode_long):
        segments of segment_frames output frames run as concurrent virtual
        streams, bit-identical to a sequential decode.  data: bytes /
        np.uint8 / torch.uint8 (host or device).  pcm: None (allocate host)
        or [max_frames, 2304] int16 (float32 with f32=True) array/tensor.
        Returns (pcm[:n], infos[:n], StreamInfo)."""
        nbytes = data.numel() if hasattr(data, "numel") else len(data)
        if max_frames is None:
            if pcm is not None or infos is not None:
                max_frames = min(len(x) for x in (pcm, infos) if x is not None)
            else:  # exact: the host frame walk of the plan
                host = data.cpu().numpy().tobytes() if hasattr(data, "cpu") else bytes(data)
                max_frames = len(long_plan(host, segment_frames, max_frame_slots(nbytes))[0])
        for x in (pcm, infos):
            if x is not None and len(x) < max_frames:
                raise ValueError("pcm / infos hold %d rows < max_frames %d" % (len(x), max_frames))
        max_frames = max(1, int(max_frames))
        if pcm is None:
            pcm = np.zeros((max_frames, 2304), np.float32 if f32 else np.int16)
        if infos is None:
            infos = np.zeros(max_frames, FRAME_INFO_DT)
        dp, k1 = _ptr(data)
        pp, k2 = _ptr(pcm)
        ip, k3 = _ptr(infos)
        n = ctypes.c_longlong()
        si = StreamInfo()
        self._ck(self._L.mp3d_batch_decode_long(self._h, dp, nbytes, int(segment_frames), pp, int(f32), int(max_frames),
                                            ip, ctypes.byref(n), ctypes.byref(si)))
        return pcm[: n.value], infos[: n.value], si

    def decode_long_packed(self, data, out_hz, out_channels, segment_frames=32, out=None, f32=True, gapless=True):
        """Frame-parallel decode of ONE long stream straight to interleaved
        PCM at out_hz / out_channels (mp3d_batch_decode_long_packed): channel
        map, gapless trim (gapless=True and a LAME tag) and resampling run on
        the GPU.  data as in decode_long.  out: None (allocate a host array of
        long_packed_bound samples) or a float32 (int16 with f32=False)
        array/tensor [cap, out_channels], host or device.  Returns
        (out[:n], StreamInfo, in_hz); raises MP3DError -5 when out is too
        small (its first cap samples are valid then)."""
        nbytes = data.numel() if hasattr(data, "numel") else len(data)
        if out is None:
            host = data.cpu().numpy().tobytes() if hasattr(data, "cpu") else bytes(data)
            out = np.zeros((long_packed_bound(host, out_hz), int(out_channels)), np.float32 if f32 else np.int16)
        dp, k1 = _ptr(data)
        op, k2 = _ptr(out)
        n, hz, si = ctypes.c_longlong(), ctypes.c_int(), StreamInfo()
        self._ck(self._L.mp3d_batch_decode_long_packed(self._h, dp, nbytes, int(segment_frames), int(out_hz),
                                                       int(out_channels), op, int(bool(f32)), len(out),
                                                       ctypes.byref(n), LONG_GAPLESS if gapless else 0,
                                                       ctypes.byref(si), ctypes.byref(hz)))
        return out[: n.value], si, hz.value

    def huffman_only(self, frames, offsets, sizes, frames_per_stream):
        head, n, F, _, keep = self._decode_head(frames, offsets, sizes, frames_per_stream)
        is_out = np.zeros((n, F, 2, 2, 576), np.int16)
        sf_out = np.zeros((n, F, 2, 2, 40), np.uint8)
        self._ck(self._L.mp3d_batch_huffman_only(*head, is_out.ctypes.data, sf_out.ctypes.data, None))
        return is_out, sf_out

    def synth_only(self, xr, block_type, mixed, nch, hz, pcm=None, stream=None):
        """xr f32 [n, F, 2, nch, 576]; block_type/mixed uint8 [n, F, 2, nch]."""
        n, F = int(xr.shape[0]), int(xr.shape[1])
        if pcm is None:
            pcm = np.zeros((n, F, 2304), np.int16)
        xp, k1 = _ptr(xr)
        bp, k2 = _ptr(block_type)
        mp, k3 = _ptr(mixed)
        pp, k4 = _ptr(pcm)
        self._ck(self._L.mp3d_batch_synth_only(self._h, xp, bp, mp, n, F, int(nch), int(hz), pp, _stream(stream)))
        return pcm


def state_bytes():
    """Bytes of one stream's opaque decoder state (mp3d_state_bytes)."""
    return int(lib().mp3d_state_bytes())


def resample_filter(in_hz, out_hz):
    """The packed sink's polyphase filter (mp3d_resample_filter; no GPU
    needed): (L, M, taps float32 [L, T])."""
    L, M, T = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    n = _check(lib().mp3d_resample_filter(int(in_hz), int(out_hz), ctypes.byref(L), ctypes.byref(M), ctypes.byref(T),
                                          None, 0))
    taps = np.zeros(n, np.float32)
    _check(lib().mp3d_resample_filter(int(in_hz), int(out_hz), None, None, None, taps.ctypes.data, taps.size))
    return L.value, M.value, taps.reshape(L.value, T.value)


def packed_max_samples(out_hz, frames, min_in_hz=8000):
    """Smallest stride of decode_packed that can never overflow for streams
    of input rate >= min_in_hz (mp3d_packed_max_samples)."""
    return int(_check(lib().mp3d_packed_max_samples(int(out_hz), int(frames), int(min_in_hz))))


def mel_filterbank(n_mels):
    """The feature sink's Slaney mel filterbank (mp3d_mel_filterbank; no GPU
    needed): float32 [n_mels, 201] over the bins f_k = 40 k Hz."""
    n = _check(lib().mp3d_mel_filterbank(int(n_mels), None, 0))
    fb = np.zeros(n, np.float32)
    _check(lib().mp3d_mel_filterbank(int(n_mels), fb.ctypes.data, fb.size))
    return fb.reshape(int(n_mels), 201)


def feat_max_frames(frames, min_in_hz=8000):
    """Smallest stride of decode_features that can never overflow for streams
    of input rate >= min_in_hz (mp3d_feat_max_frames)."""
    return int(_check(lib().mp3d_feat_max_frames(int(frames), int(min_in_hz))))


def loudness_filter(hz):
    """The loudness sink's K-weighting at rate hz (mp3d_loudness_filter; no
    GPU needed): float64 [2, 5], b0 b1 b2 a1 a2 of the shelf and the high-pass."""
    c = np.zeros(10, np.float64)
    _check(lib().mp3d_loudness_filter(int(hz), c.ctypes.data, c.size))
    return c.reshape(2, 5)


def loud_max_blocks(hz, frames, min_in_hz=8000):
    """Smallest stride of decode_loudness that can never overflow for streams
    of input rate >= min_in_hz (mp3d_loud_max_blocks)."""
    return int(_check(lib().mp3d_loud_max_blocks(int(hz), int(frames), int(min_in_hz))))


def integrated_lufs(z):
    """Gated integrated loudness (BS.1770-4) of a sequence of 100 ms block
    energies (mp3d_loudness_integrated; no GPU needed): float, -inf when
    fewer than 4 blocks or none passes the gates."""
    z = np.ascontiguousarray(z, np.float32).reshape(-1)
    out = ctypes.c_double()
    _check(lib().mp3d_loudness_integrated(z.ctypes.data if z.size else None, z.size, ctypes.byref(out)))
    return float(out.value)


def truepeak_filter():
    """The true-peak tap's 4x oversampling filter (mp3d_truepeak_filter; no
    GPU needed): float32 [4, 12], row p the taps of phase p."""
    t = np.zeros((4, 12), np.float32)
    _check(lib().mp3d_truepeak_filter(t.ctypes.data, t.size))
    return t


def stretch_window(hz):
    """The tempo sink's crossfade table at rate hz (mp3d_stretch_window; no
    GPU needed): float32 [H], H = (hz + 50) // 100."""
    H = int(_check(lib().mp3d_stretch_window(int(hz), None, 0)))
    w = np.zeros(H, np.float32)
    _check(lib().mp3d_stretch_window(int(hz), w.ctypes.data, w.size))
    return w


def stretch_max_samples(hz, in_samples, num=1, den=2):
    """Smallest stride of stretch that can never overflow for one call
    feeding in_samples samples at tempo num / den (mp3d_stretch_max_samples)."""
    return int(_check(lib().mp3d_stretch_max_samples(int(hz), int(in_samples), int(num), int(den))))


def _eq_bands(bands):
    """(type, f0_hz, gain_db, q) tuples as an array of mp3d_eq_band"""
    bands = [] if bands is None else list(bands)
    arr = np.zeros(len(bands), EQ_BAND_DT)
    for k, (t, f0, g, q) in enumerate(bands):
        arr[k] = (int(t), float(f0), float(g), float(q))
    return arr


def eq_design(hz, bands, preamp_db=0.0):
    """The biquads of an equaliser curve at rate hz (mp3d_eq_design; no GPU
    needed): float64 [n, 5], row k = b0 b1 b2 a1 a2 of stage k.  bands and
    preamp_db as in BatchDecoder.set_eq."""
    arr = _eq_bands(bands)
    coef = np.zeros((arr.size, 5), np.float64)
    _check(lib().mp3d_eq_design(int(hz), arr.ctypes.data if arr.size else None, arr.size, float(preamp_db),
                                coef.ctypes.data, coef.size))
    return coef


def limiter_lookahead(hz):
    """The limiter's look-ahead A = (hz + 50) // 100 in samples at rate hz
    (mp3d_limiter_lookahead; no GPU needed)."""
    return int(_check(lib().mp3d_limiter_lookahead(int(hz))))


def limiter_max_samples(hz, in_samples):
    """Smallest stride of limit that can never overflow for one call feeding
    in_samples samples (mp3d_limiter_max_samples): in_samples + A + 6."""
    return int(_check(lib().mp3d_limiter_max_samples(int(hz), int(in_samples))))


def segment_threshold(hz, db):
    """The segment sink's threshold for a mean square of db dBFS (-96 .. 0) at
    rate hz, as a hop energy (mp3d_segment_threshold; no GPU needed)."""
    return int(_check(lib().mp3d_segment_threshold(int(hz), float(db))))


def segment_max(hz, in_samples, pause_hops, speech_hops):
    """Smallest stride of segments that can never overflow for one call
    feeding in_samples samples (mp3d_segment_max)."""
    return int(_check(lib().mp3d_segment_max(int(hz), int(in_samples), int(pause_hops), int(speech_hops))))


def long_packed_bound(data, out_hz):
    """Upper bound of the samples per channel decode_long_packed writes for
    this stream at out_hz (mp3d_long_packed_bound; host bytes, no GPU)."""
    data = bytes(data)
    return int(_check(lib().mp3d_long_packed_bound(data, len(data), int(out_hz))))


def max_frame_slots(nbytes):
    """Upper bound on the frame slots in nbytes of stream: the smallest
    Layer III frame is 24 B (MPEG-2 LSF, 8 kbps at 24 kHz; MPEG-1: 96 B)."""
    return int(nbytes) // 24 + 2


def pitch_span(hz, fmin, fmax):
    """(SPAN, tmin, tmax) of the pitch sink at rate hz for the limits fmin and
    fmax in Hz: the samples a frame reads and its lag range
    (mp3d_pitch_span; no GPU needed)."""
    lo, hi = ctypes.c_int(), ctypes.c_int()
    span = _check(lib().mp3d_pitch_span(int(hz), int(fmin), int(fmax), ctypes.byref(lo), ctypes.byref(hi)))
    return int(span), lo.value, hi.value


def pitch_max_frames(hz, in_samples, fmin):
    """Smallest stride of pitch records that can never overflow for one call
    feeding in_samples samples (mp3d_pitch_max_frames)."""
    return int(_check(lib().mp3d_pitch_max_frames(int(hz), int(in_samples), int(fmin))))


def long_plan(data, segment_frames=32, max_frames=None):
    """Host-side segment plan of BatchDecoder.decode_long (mp3d_long_plan;
    no GPU needed).  Returns (frame_off [n] uint64, seg_start [K] int64,
    max_warmup)."""
    data = bytes(data)
    if max_frames is None:
        max_frames = max_frame_slots(len(data))
    L = int(segment_frames)
    off = np.zeros(max_frames, np.uint64)
    seg = np.zeros(max_frames // max(L, 1) + 2, np.int64)
    n, w = ctypes.c_longlong(), ctypes.c_int()
    _check(lib().mp3d_long_plan(data, len(data), L, int(max_frames), off.ctypes.data, seg.ctypes.data,
                                ctypes.byref(n), ctypes.byref(w)))
    k = (n.value + L - 1) // L
    return off[: n.value], seg[:k], w.value


def pcm_to_planar(pcm_frames, infos):
    """[F, 2304] int16/float32 + infos [F] -> [channels, samples] for frames
    with audio (1152 samples per channel, 576 for an MPEG-2 / 2.5 LSF frame,
    interleaved at the start of the frame's row)."""
    rows = []
    nch = 0
    for f in range(pcm_frames.shape[0]):
        n = int(infos[f]["samples"])
        if n:
            nch = int(infos[f]["channels"])
            rows.append(pcm_frames[f, : n * nch].reshape(n, nch))
    if not rows:
        return np.zeros((0, 0), pcm_frames.dtype)
    return np.concatenate(rows).T.copy()


def gapless_trim(planar, info):
    """Apply a stream's gapless trim (StreamInfo or its dict) to planar PCM
    [channels, samples] holding every decoded sample from the stream start:
    FFmpeg semantics (libavformat/mp3dec.c) -- drop the first skip_samples,
    and everything from end_sample on when the tag gives a frame count."""
    get = info.get if isinstance(info, dict) else (lambda k: getattr(info, k))
    if not get("has_lame"):
        return planar
    end = get("end_sample")
    stop = planar.shape[1] if end is None or end < 0 else min(int(end), planar.shape[1])
    return planar[:, int(get("skip_samples")):stop]
