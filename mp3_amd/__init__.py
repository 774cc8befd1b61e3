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
"""
import contextlib
import ctypes
import os
import pathlib

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ["MP3D_LIB"]) if os.environ.get("MP3D_LIB") else _HERE / "libmp3d.so"

MP3D_E = {0: "ok", -1: "bad argument", -2: "no usable HIP device", -3: "HIP runtime error", -4: "out of memory",
          -5: "batch exceeds handle capacity", -6: "no complete frame in buffer"}


class FrameInfo(ctypes.Structure):
    _fields_ = [("frame_bytes", ctypes.c_int), ("channels", ctypes.c_int), ("hz", ctypes.c_int),
                ("layer", ctypes.c_int), ("bitrate_kbps", ctypes.c_int), ("samples", ctypes.c_int)]


class StreamInfo(ctypes.Structure):
    """mp3d_stream_info: leading Xing/Info tag and FFmpeg-style gapless trim."""
    _fields_ = [("has_tag", ctypes.c_int), ("has_lame", ctypes.c_int), ("enc_delay", ctypes.c_int),
                ("enc_padding", ctypes.c_int), ("total_frames", ctypes.c_int), ("skip_samples", ctypes.c_int),
                ("end_sample", ctypes.c_longlong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


FRAME_INFO_DT = np.dtype([("frame_bytes", np.int32), ("channels", np.int32), ("hz", np.int32),
                          ("layer", np.int32), ("bitrate_kbps", np.int32), ("samples", np.int32)])

EXPORTS = ["mp3d_dec_create", "mp3d_dec_create_on", "mp3d_dec_destroy", "mp3d_dec_reset", "mp3d_decode_frame",
           "mp3d_decode_frame_f32", "mp3d_batch_decode_f32",
           "mp3d_batch_create", "mp3d_batch_destroy", "mp3d_batch_reset", "mp3d_batch_decode", "mp3d_batch_sync",
           "mp3d_batch_huffman_only", "mp3d_batch_synth_only", "mp3d_strerror", "mp3d_last_hip_error",
           "mp3d_abi_version", "mp3d_batch_set_timing", "mp3d_batch_kernel_times", "mp3d_batch_stream_info",
           "mp3d_dec_stream_info", "mp3d_batch_decode_long",
           "mp3d_long_plan", "mp3d_batch_set_options", "mp3d_dec_set_options", "mp3d_decode_frame_ex",
           "mp3d_state_bytes", "mp3d_batch_get_state", "mp3d_batch_set_state", "mp3d_dec_get_state",
           "mp3d_dec_set_state", "mp3d_resample_filter", "mp3d_batch_set_output", "mp3d_packed_max_samples",
           "mp3d_batch_decode_packed", "mp3d_batch_resample_time", "mp3d_batch_decode_long_packed",
           "mp3d_long_packed_bound", "mp3d_mel_filterbank", "mp3d_feat_max_frames", "mp3d_batch_set_features",
           "mp3d_batch_decode_features", "mp3d_batch_features", "mp3d_batch_feature_time", "mp3d_batch_set_window",
           "mp3d_batch_sink_window", "mp3d_loudness_filter", "mp3d_loud_max_blocks", "mp3d_batch_set_loudness",
           "mp3d_batch_loudness", "mp3d_batch_decode_loudness", "mp3d_loudness_integrated",
           "mp3d_batch_loudness_integrated", "mp3d_batch_loudness_time", "mp3d_truepeak_filter",
           "mp3d_batch_set_true_peak", "mp3d_batch_true_peak", "mp3d_batch_decode_measure",
           "mp3d_batch_normalize_gain", "mp3d_batch_apply_gain", "mp3d_batch_true_peak_time", "mp3d_stretch_window",
           "mp3d_stretch_max_samples", "mp3d_batch_set_stretch", "mp3d_batch_set_tempo", "mp3d_batch_stretch",
           "mp3d_batch_decode_stretched", "mp3d_batch_stretch_time", "mp3d_limiter_lookahead",
           "mp3d_limiter_max_samples", "mp3d_batch_set_limiter", "mp3d_batch_limit", "mp3d_batch_decode_limited",
           "mp3d_batch_limiter_time", "mp3d_segment_threshold", "mp3d_segment_max", "mp3d_batch_set_segments",
           "mp3d_batch_set_segment_threshold", "mp3d_batch_segments", "mp3d_batch_decode_segments",
           "mp3d_batch_segment_time", "mp3d_eq_design", "mp3d_batch_set_eq", "mp3d_batch_eq",
           "mp3d_batch_decode_equalized", "mp3d_batch_eq_time"]

OPT_CRC_CHECK = 1  # MP3D_OPT_CRC_CHECK: drop frames whose CRC-16 mismatches
LONG_GAPLESS = 1  # MP3D_LONG_GAPLESS: apply the LAME tag's trim inside decode_long_packed
PACK_FLUSH = 1  # MP3D_PACK_FLUSH: feed zeros after the call's frames, then restart the resamplers
PACK_GAPLESS = 2  # MP3D_PACK_GAPLESS: fix an unfixed sample window from the stream's LAME tag (decode_packed/_features)
WINDOW_NO_END = 2**63 - 1  # MP3D_WINDOW_NO_END: a sample window without an end
FEAT_LOG10 = 1  # MP3D_FEAT_LOG10: log10(max(mel, 1e-10)) instead of the mel energies
MP3D_FEAT_LOG10 = FEAT_LOG10
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
FRAME_F32, FRAME_LAST = 1, 2  # mp3d_decode_frame_ex flags

_lib = None


class MP3DError(RuntimeError):
    pass


def _bind(L):
    """Argument and result types of every export, on one loaded build."""
    vp, i, u64p, u32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p
    L.mp3d_dec_create.argtypes = [ctypes.POINTER(vp)]
    L.mp3d_dec_create_on.argtypes = [i, ctypes.POINTER(vp)]
    L.mp3d_dec_destroy.argtypes = [vp]
    L.mp3d_dec_destroy.restype = None
    L.mp3d_dec_reset.argtypes = [vp]
    L.mp3d_dec_reset.restype = None
    L.mp3d_decode_frame.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, vp, ctypes.POINTER(FrameInfo)]
    L.mp3d_batch_create.argtypes = [i, i, i, ctypes.POINTER(vp)]
    L.mp3d_batch_destroy.argtypes = [vp]
    L.mp3d_batch_destroy.restype = None
    L.mp3d_batch_reset.argtypes = [vp]
    L.mp3d_batch_decode.argtypes = [vp, vp, u64p, u32p, i, i, vp, vp, vp]
    L.mp3d_batch_decode_f32.argtypes = [vp, vp, u64p, u32p, i, i, vp, vp, vp]
    L.mp3d_decode_frame_f32.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, vp, ctypes.POINTER(FrameInfo)]
    L.mp3d_batch_sync.argtypes = [vp]
    L.mp3d_batch_huffman_only.argtypes = [vp, vp, u64p, u32p, i, i, vp, vp, vp]
    L.mp3d_batch_synth_only.argtypes = [vp, vp, vp, vp, i, i, i, i, vp, vp]
    L.mp3d_strerror.argtypes = [i]
    L.mp3d_strerror.restype = ctypes.c_char_p
    L.mp3d_batch_set_timing.argtypes = [vp, i]
    L.mp3d_batch_kernel_times.argtypes = [vp, vp]
    L.mp3d_batch_stream_info.argtypes = [vp, i, vp]
    L.mp3d_dec_stream_info.argtypes = [vp, ctypes.POINTER(StreamInfo)]
    L.mp3d_batch_decode_long.argtypes = [vp, vp, ctypes.c_size_t, i, vp, i, ctypes.c_longlong, vp,
                                         ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(StreamInfo)]
    L.mp3d_long_plan.argtypes = [ctypes.c_char_p, ctypes.c_size_t, i, ctypes.c_longlong, vp, vp,
                                 ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)]
    L.mp3d_batch_set_options.argtypes = [vp, i]
    L.mp3d_dec_set_options.argtypes = [vp, i]
    L.mp3d_decode_frame_ex.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, vp, i, ctypes.POINTER(FrameInfo)]
    L.mp3d_state_bytes.restype = ctypes.c_size_t
    L.mp3d_batch_get_state.argtypes = [vp, i, i, vp]
    L.mp3d_batch_set_state.argtypes = [vp, i, i, vp]
    L.mp3d_dec_get_state.argtypes = [vp, vp]
    L.mp3d_dec_set_state.argtypes = [vp, vp]
    ip = ctypes.POINTER(ctypes.c_int)
    L.mp3d_resample_filter.argtypes = [i, i, ip, ip, ip, vp, ctypes.c_size_t]
    L.mp3d_resample_filter.restype = ctypes.c_longlong
    L.mp3d_batch_set_output.argtypes = [vp, i, i]
    L.mp3d_packed_max_samples.argtypes = [i, i, i]
    L.mp3d_packed_max_samples.restype = ctypes.c_longlong
    L.mp3d_batch_decode_packed.argtypes = [vp, vp, u64p, u32p, i, i, vp, i, ctypes.c_longlong, vp, i, vp, vp]
    L.mp3d_batch_resample_time.argtypes = [vp, vp]
    L.mp3d_batch_decode_long_packed.argtypes = [vp, vp, ctypes.c_size_t, i, i, i, vp, i, ctypes.c_longlong,
                                                ctypes.POINTER(ctypes.c_longlong), i, ctypes.POINTER(StreamInfo), ip]
    L.mp3d_long_packed_bound.argtypes = [ctypes.c_char_p, ctypes.c_size_t, i]
    L.mp3d_long_packed_bound.restype = ctypes.c_longlong
    L.mp3d_mel_filterbank.argtypes = [i, vp, ctypes.c_size_t]
    L.mp3d_mel_filterbank.restype = ctypes.c_longlong
    L.mp3d_feat_max_frames.argtypes = [i, i]
    L.mp3d_feat_max_frames.restype = ctypes.c_longlong
    L.mp3d_batch_set_features.argtypes = [vp, i, i]
    L.mp3d_batch_decode_features.argtypes = [vp, vp, u64p, u32p, i, i, vp, ctypes.c_longlong, vp, i, vp, vp]
    L.mp3d_batch_features.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, ctypes.c_longlong, vp, i, vp]
    L.mp3d_batch_feature_time.argtypes = [vp, vp]
    if hasattr(L, "mp3d_batch_set_window"):  # (an older build loaded for an A/B lacks the two)
        L.mp3d_batch_set_window.argtypes = [vp, i, i, vp, vp]
        L.mp3d_batch_sink_window.argtypes = [vp, i, i, vp, vp, vp]
    if hasattr(L, "mp3d_batch_set_loudness"):  # (an older build loaded for an A/B lacks the loudness sink)
        L.mp3d_loudness_filter.argtypes = [i, vp, ctypes.c_size_t]
        L.mp3d_loudness_filter.restype = ctypes.c_longlong
        L.mp3d_loud_max_blocks.argtypes = [i, i, i]
        L.mp3d_loud_max_blocks.restype = ctypes.c_longlong
        L.mp3d_batch_set_loudness.argtypes = [vp, i]
        L.mp3d_batch_loudness.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, ctypes.c_longlong, vp, vp, i, vp]
        L.mp3d_batch_decode_loudness.argtypes = [vp, vp, u64p, u32p, i, i, vp, ctypes.c_longlong, vp, vp, i, vp, vp]
        L.mp3d_loudness_integrated.argtypes = [vp, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)]
        L.mp3d_batch_loudness_integrated.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, vp]
        L.mp3d_batch_loudness_time.argtypes = [vp, vp]
    if hasattr(L, "mp3d_batch_set_true_peak"):  # (an older build loaded for an A/B lacks true peak and gain)
        L.mp3d_truepeak_filter.argtypes = [vp, ctypes.c_size_t]
        L.mp3d_truepeak_filter.restype = ctypes.c_longlong
        L.mp3d_batch_set_true_peak.argtypes = [vp, i]
        L.mp3d_batch_true_peak.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, i, vp]
        L.mp3d_batch_decode_measure.argtypes = [vp, vp, u64p, u32p, i, i, vp, ctypes.c_longlong, vp, vp, vp, i, vp, vp]
        L.mp3d_batch_normalize_gain.argtypes = [vp, vp, vp, i, ctypes.c_double, ctypes.c_double, vp, vp]
        L.mp3d_batch_apply_gain.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, vp, i, vp]
        L.mp3d_batch_true_peak_time.argtypes = [vp, vp]
    if hasattr(L, "mp3d_batch_set_stretch"):  # (an older build loaded for an A/B lacks the tempo sink)
        L.mp3d_stretch_window.argtypes = [i, vp, ctypes.c_size_t]
        L.mp3d_stretch_window.restype = ctypes.c_longlong
        L.mp3d_stretch_max_samples.argtypes = [i, ctypes.c_longlong, i, i]
        L.mp3d_stretch_max_samples.restype = ctypes.c_longlong
        L.mp3d_batch_set_stretch.argtypes = [vp, i]
        L.mp3d_batch_set_tempo.argtypes = [vp, i, i, vp, vp]
        L.mp3d_batch_stretch.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, ctypes.c_longlong, vp, i, vp]
        L.mp3d_batch_decode_stretched.argtypes = [vp, vp, u64p, u32p, i, i, vp, ctypes.c_longlong, vp, i, vp, vp]
        L.mp3d_batch_stretch_time.argtypes = [vp, vp]
    if hasattr(L, "mp3d_batch_set_limiter"):  # (an older build loaded for an A/B lacks the limiter)
        L.mp3d_limiter_lookahead.argtypes = [i]
        L.mp3d_limiter_lookahead.restype = ctypes.c_longlong
        L.mp3d_limiter_max_samples.argtypes = [i, ctypes.c_longlong]
        L.mp3d_limiter_max_samples.restype = ctypes.c_longlong
        L.mp3d_batch_set_limiter.argtypes = [vp, i, ctypes.c_double]
        L.mp3d_batch_limit.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, vp, i, ctypes.c_longlong, vp, vp, i, vp]
        L.mp3d_batch_decode_limited.argtypes = [vp, vp, u64p, u32p, i, i, vp, vp, i, ctypes.c_longlong, vp, vp, i, vp,
                                                vp]
        L.mp3d_batch_limiter_time.argtypes = [vp, vp]
    if hasattr(L, "mp3d_batch_set_segments"):  # (an older build loaded for an A/B lacks the segment sink)
        L.mp3d_segment_threshold.argtypes = [i, ctypes.c_double]
        L.mp3d_segment_threshold.restype = ctypes.c_longlong
        L.mp3d_segment_max.argtypes = [i, ctypes.c_longlong, i, i]
        L.mp3d_segment_max.restype = ctypes.c_longlong
        L.mp3d_batch_set_segments.argtypes = [vp, i, i, i, i]
        L.mp3d_batch_set_segment_threshold.argtypes = [vp, i, i, vp]
        L.mp3d_batch_segments.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, ctypes.c_longlong, vp, i, vp]
        L.mp3d_batch_decode_segments.argtypes = [vp, vp, u64p, u32p, i, i, vp, ctypes.c_longlong, vp, i, vp, vp]
        L.mp3d_batch_segment_time.argtypes = [vp, vp]
    if hasattr(L, "mp3d_batch_set_eq"):  # (an older build loaded for an A/B lacks the equaliser)
        L.mp3d_eq_design.argtypes = [i, vp, i, ctypes.c_double, vp, ctypes.c_size_t]
        L.mp3d_eq_design.restype = ctypes.c_longlong
        L.mp3d_batch_set_eq.argtypes = [vp, vp, i, ctypes.c_double]
        L.mp3d_batch_eq.argtypes = [vp, vp, ctypes.c_longlong, vp, i, vp, ctypes.c_longlong, vp, i, vp]
        L.mp3d_batch_decode_equalized.argtypes = [vp, vp, u64p, u32p, i, i, vp, ctypes.c_longlong, vp, i, vp, vp]
        L.mp3d_batch_eq_time.argtypes = [vp, vp]
    if hasattr(L, "mp3d_debug_wglds_probe"):  # libmp3d_wglds.so only (tests/test_gpu_wglds.py)
        L.mp3d_debug_wglds_probe.argtypes = [i, i, vp, i]
    return L


_loaded = {}  # path -> CDLL: one copy of a build per process


def _load(path):
    path = pathlib.Path(path).resolve()
    if path not in _loaded:
        if not path.exists():
            raise ImportError("mp3_amd: %s missing -- run __graft_entry__.build() (no CPU fallback exists)" % path)
        _loaded[path] = _bind(ctypes.CDLL(str(path)))
    return _loaded[path]


def lib():
    """The current build of the library: libmp3d.so (or MP3D_LIB) unless
    inside library().  Fails loudly if it was not built."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


@contextlib.contextmanager
def library(path):
    """Make lib() return the build at `path` inside the block (a debug build
    next to the product in one process).  A Decoder / BatchDecoder keeps the
    build that created its handle for every later call, whatever is current
    then; the module-level functions use the current one."""
    global _lib
    prev, _lib = _lib, _load(path)
    try:
        yield _lib
    finally:
        _lib = prev


def _check(rc, L=None):
    if rc < 0:
        L = L or lib()
        raise MP3DError("mp3d error %d (%s), hip error %d" % (rc, L.mp3d_strerror(rc).decode(), L.mp3d_last_hip_error()))
    return rc


def _ptr(x):
    """(pointer, keepalive) for a numpy array, torch tensor, bytes or None."""
    if x is None:
        return None, None
    if isinstance(x, (bytes, bytearray)):
        a = np.frombuffer(bytes(x), np.uint8)
        return a.ctypes.data, a
    if isinstance(x, np.ndarray):
        if not x.flags.c_contiguous:
            raise ValueError("array must be C-contiguous")
        return x.ctypes.data, x
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr(), x
    raise TypeError("unsupported buffer type %r" % type(x))


def _pack_flags(flush, gapless=False):
    return (PACK_FLUSH if flush else 0) | (PACK_GAPLESS if gapless else 0)


def _stream(stream):
    """A HIP stream handle (int) as a call's hip_stream argument; None / 0: the handle's own stream."""
    return ctypes.c_void_p(stream) if stream else None


class Decoder:
    """Per-frame decoder (mp3d_decode_frame), one per stream."""

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
        if getattr(self, "_h", None):
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
        if getattr(self, "_h", None):
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

    def decode(self, frames, offsets, sizes, frames_per_stream, pcm=None, infos=None, stream=None, f32=False):
        """frames: bytes/np.uint8/torch.uint8; pcm: None (allocate host) or
        int16 (float32 with f32=True) array/tensor [n, F, 2304]; infos: None
        or FRAME_INFO_DT array / int32 tensor [n, F, 6].  Returns (pcm, infos)."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        if pcm is None:
            pcm = np.zeros((n, F, 2304), np.float32 if f32 else np.int16)
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        pp, k2 = _ptr(pcm)
        ip, k3 = _ptr(infos)
        fn = self._L.mp3d_batch_decode_f32 if f32 else self._L.mp3d_batch_decode
        self._ck(fn(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, pp, ip, _stream(stream)))
        return pcm, infos

    def set_output(self, hz, channels):
        """Format of the packed sink (decode_packed): hz from RATES, channels
        1 or 2; hz = 0 turns the sink off and frees its buffers.  A change
        restarts every stream's resampler."""
        self._ck(self._L.mp3d_batch_set_output(self._h, int(hz), int(channels)))
        self._out = (int(hz), int(channels))
        self._mels = 0  # a change of the output format turns the feature sink off
        self._loud = False  # and the loudness sink
        self._tp = False  # and the true-peak tap
        self._stretch = False  # and the tempo sink
        self._limit = None  # and the limiter (its ceiling in dBTP while it is on)
        self._segments = None  # and the segment sink (its pause and shortest segment in hops while it is on)
        self._eq = 0  # and the equaliser (its number of bands while it is on)

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
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        hz, ch = getattr(self, "_out", (0, 0))
        if stride is None:  # (no format set: the call below fails with MP3D_E_ARG)
            stride = int(out.shape[1]) if out is not None else packed_max_samples(hz, F) if hz else 1
        stride = int(stride)
        if out is None:
            out = np.zeros((n, stride, ch), np.float32 if f32 else np.int16)
        if counts is None:
            counts = np.zeros(n, np.int32)
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        op, k2 = _ptr(out)
        cp, k3 = _ptr(counts)
        ip, k4 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_packed(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, op, int(bool(f32)),
                                              stride, cp,
                                              _pack_flags(flush, gapless), ip, _stream(stream)))
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

    def _feat_args(self, n, feat, counts, stride, default_stride):
        nm = getattr(self, "_mels", 0)
        if stride is None:  # (features off: the call fails with MP3D_E_ARG)
            stride = int(feat.shape[1]) if feat is not None else default_stride() if nm else 1
        stride = int(stride)
        if feat is None:
            feat = np.zeros((n, stride, max(nm, 1)), np.float32)
        if counts is None:
            counts = np.zeros(n, np.int32)
        return feat, counts, stride

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
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        feat, counts, stride = self._feat_args(n, feat, counts, stride, lambda: feat_max_frames(F))
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        op, k2 = _ptr(feat)
        cp, k3 = _ptr(counts)
        ip, k4 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_features(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, op, stride, cp,
                                                    _pack_flags(flush, gapless), ip, _stream(stream)))
        return feat, counts, infos

    def features(self, samples, counts, feat=None, feat_counts=None, flush=False, stride=None, stream=None):
        """The feature stage alone (mp3d_batch_features): samples float32
        [n, sample_stride] 16 kHz mono, counts int32 [n] samples per stream
        (both host arrays or device tensors), through the same kernels and
        per-stream state as decode_features.  Returns (feat, feat_counts)."""
        n, ss = int(samples.shape[0]), int(samples.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        feat, feat_counts, stride = self._feat_args(n, feat, feat_counts, stride, lambda: (ss + 200 + 159) // 160 + 1)
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        op, k3 = _ptr(feat)
        fc, k4 = _ptr(feat_counts)
        self._ck(self._L.mp3d_batch_features(self._h, sp if ss else None, ss, cp, n, op, stride, fc,
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

    def _loud_args(self, n, blocks, counts, peak, stride, default_stride):
        if stride is None:  # (loudness off: the call fails with MP3D_E_ARG)
            stride = int(blocks.shape[1]) if blocks is not None else default_stride() if getattr(self, "_loud", 0) else 1
        stride = int(stride)
        if blocks is None:
            blocks = np.zeros((n, stride), np.float32)
        if counts is None:
            counts = np.zeros(n, np.int32)
        if peak is None:
            peak = np.zeros(n, np.float32)
        return blocks, counts, peak, stride

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
        n, ss = int(samples.shape[0]), int(samples.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        H = (getattr(self, "_out", (0, 0))[0] + 5) // 10
        blocks, block_counts, peak, stride = self._loud_args(n, blocks, block_counts, peak, stride,
                                                             lambda: (H - 1 + ss) // H)
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        op, k3 = _ptr(blocks)
        bc, k4 = _ptr(block_counts)
        pp, k5 = _ptr(peak)
        self._ck(self._L.mp3d_batch_loudness(self._h, sp if ss else None, ss, cp, n, op, stride, bc, pp,
                                             _pack_flags(flush), _stream(stream)))
        return blocks, block_counts, peak

    def decode_loudness(self, frames, offsets, sizes, frames_per_stream, blocks=None, counts=None, peak=None,
                        infos=None, flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does and write every stream's block
        energies and sample peak (mp3d_batch_decode_loudness).  stride
        defaults to blocks', else to loud_max_blocks.  flush and gapless as in
        decode_packed; the flush also drops the open block.  Returns (blocks,
        counts, peak, infos)."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        hz = getattr(self, "_out", (0, 0))[0]
        blocks, counts, peak, stride = self._loud_args(n, blocks, counts, peak, stride, lambda: loud_max_blocks(hz, F))
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        op, k2 = _ptr(blocks)
        cp, k3 = _ptr(counts)
        pp, k4 = _ptr(peak)
        ip, k5 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_loudness(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, op, stride, cp, pp,
                                                    _pack_flags(flush, gapless), ip, _stream(stream)))
        return blocks, counts, peak, infos

    def integrated_lufs(self, blocks, counts, lufs=None, stream=None):
        """Gated integrated loudness of every row of blocks float32
        [n, stride] holding counts[s] block energies, on the GPU
        (mp3d_batch_loudness_integrated); host arrays or device tensors.
        Returns lufs float32 [n], -inf for a row of fewer than 4 blocks."""
        n, stride = int(blocks.shape[0]), int(blocks.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        if lufs is None:
            lufs = np.zeros(n, np.float32)
        bp, k1 = _ptr(blocks)
        cp, k2 = _ptr(counts)
        lp, k3 = _ptr(lufs)
        self._ck(self._L.mp3d_batch_loudness_integrated(self._h, bp if stride else None, stride, cp, n, lp,
                                                        _stream(stream)))
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
        n, ss = int(samples.shape[0]), int(samples.shape[1]) if stride is None else int(stride)
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        if tpeak is None:
            tpeak = np.zeros(n, np.float32)
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        tp, k3 = _ptr(tpeak)
        self._ck(self._L.mp3d_batch_true_peak(self._h, sp if ss else None, ss, cp, n, tp, _pack_flags(flush),
                                              _stream(stream)))
        return tpeak

    def decode_measure(self, frames, offsets, sizes, frames_per_stream, blocks=None, counts=None, peak=None,
                       tpeak=None, infos=None, flush=False, stride=None, stream=None, gapless=False):
        """decode_loudness plus the true-peak tap on the same samples
        (mp3d_batch_decode_measure); needs set_loudness and set_true_peak.
        Returns (blocks, counts, peak, tpeak, infos)."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        hz = getattr(self, "_out", (0, 0))[0]
        blocks, counts, peak, stride = self._loud_args(n, blocks, counts, peak, stride, lambda: loud_max_blocks(hz, F))
        if tpeak is None:
            tpeak = np.zeros(n, np.float32)
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        op, k2 = _ptr(blocks)
        cp, k3 = _ptr(counts)
        pp, k4 = _ptr(peak)
        tp, k5 = _ptr(tpeak)
        ip, k6 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_measure(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, op, stride, cp, pp,
                                                   tp, _pack_flags(flush, gapless), ip, _stream(stream)))
        return blocks, counts, peak, tpeak, infos

    def normalize_gain(self, lufs, tpeak=None, target=-23.0, max_dbtp=-1.0, gain=None, stream=None):
        """The gain that brings each stream from lufs[s] to target LUFS,
        limited so that gain * tpeak[s] stays at or below max_dbtp dBTP
        (mp3d_batch_normalize_gain); tpeak=None: no limit.  A stream whose
        loudness is not finite gets gain 1.  Host arrays or device tensors,
        float32 [n].  Returns gain."""
        if not hasattr(lufs, "data_ptr"):
            lufs = np.ascontiguousarray(lufs, np.float32)
        if tpeak is not None and not hasattr(tpeak, "data_ptr"):
            tpeak = np.ascontiguousarray(tpeak, np.float32)
        n = int(lufs.shape[0])
        if gain is None:
            gain = np.zeros(n, np.float32)
        lp, k1 = _ptr(lufs)
        tp, k2 = _ptr(tpeak)
        gp, k3 = _ptr(gain)
        self._ck(self._L.mp3d_batch_normalize_gain(self._h, lp, tp, n, float(target), float(max_dbtp), gp,
                                                   _stream(stream)))
        return gain

    def apply_gain(self, samples, counts, gain, out=None, f32=True, stream=None):
        """out[s, i, c] = samples[s, i, c] * gain[s] for i < counts[s]
        (mp3d_batch_apply_gain): samples float32 [n, stride, channels] in the
        packed format, counts int32 [n], gain float32 [n]; out: None (allocate
        host, zeros past the counts) or float32 (int16 with f32=False)
        array/tensor of samples' shape, which may be samples itself for
        float32.  Nothing past counts[s] is written.  Returns out."""
        n, ss = int(samples.shape[0]), int(samples.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        if not hasattr(gain, "data_ptr"):
            gain = np.ascontiguousarray(gain, np.float32)
        if out is None:
            out = np.zeros(tuple(samples.shape), np.float32 if f32 else np.int16)
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        gp, k3 = _ptr(gain)
        op, k4 = _ptr(out)
        self._ck(self._L.mp3d_batch_apply_gain(self._h, sp if ss else None, ss, cp, n, gp, op, int(bool(f32)),
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

    def _stretch_args(self, n, out, out_counts, stride, default_stride):
        hz, ch = getattr(self, "_out", (0, 0))
        if stride is None:  # (stretch off: the call fails with MP3D_E_ARG)
            stride = int(out.shape[1]) if out is not None else default_stride(hz) if getattr(self, "_stretch", 0) else 1
        stride = int(stride)
        if out is None:
            out = np.zeros((n, stride, ch), np.float32)
        if out_counts is None:
            out_counts = np.zeros(n, np.int32)
        return out, out_counts, stride

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
        n, ss = int(samples.shape[0]), int(samples.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        out, out_counts, stride = self._stretch_args(n, out, out_counts, stride,
                                                     lambda hz: stretch_max_samples(hz, ss, 1, 2))
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        op, k3 = _ptr(out)
        oc, k4 = _ptr(out_counts)
        self._ck(self._L.mp3d_batch_stretch(self._h, sp if ss else None, ss, cp, n, op, stride, oc,
                                            _pack_flags(flush), _stream(stream)))
        return out, out_counts

    def decode_stretched(self, frames, offsets, sizes, frames_per_stream, out=None, counts=None, infos=None,
                         flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        samples at its tempo (mp3d_batch_decode_stretched).  stride defaults to
        out's, else to the bound that cannot overflow at the slowest tempo.
        flush and gapless as in decode_packed; the flush also ends the
        stretch.  Returns (out, counts, infos)."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        out, counts, stride = self._stretch_args(
            n, out, counts, stride, lambda hz: stretch_max_samples(hz, packed_max_samples(hz, F), 1, 2))
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        op, k2 = _ptr(out)
        cp, k3 = _ptr(counts)
        ip, k4 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_stretched(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, op, stride, cp,
                                                     _pack_flags(flush, gapless), ip, _stream(stream)))
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

    def _limit_args(self, n, out, out_counts, gain, gr, f32, stride, default_stride):
        hz, ch = getattr(self, "_out", (0, 0))
        if stride is None:  # (limiter off: the call fails with MP3D_E_ARG)
            on = getattr(self, "_limit", None) is not None
            stride = int(out.shape[1]) if out is not None else default_stride(hz) if on else 1
        stride = int(stride)
        if out is None:
            out = np.zeros((n, stride, ch), np.float32 if f32 else np.int16)
        if out_counts is None:
            out_counts = np.zeros(n, np.int32)
        if gain is not None and not hasattr(gain, "data_ptr"):
            gain = np.ascontiguousarray(gain, np.float32)
        if gr is None:
            gr = np.ones(n, np.float32)
        return out, out_counts, gain, gr, stride

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
        n, ss = int(samples.shape[0]), int(samples.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        out, out_counts, gain, gr, stride = self._limit_args(n, out, out_counts, gain, gr, f32, stride,
                                                             lambda hz: limiter_max_samples(hz, ss))
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        gp, k3 = _ptr(gain)
        op, k4 = _ptr(out)
        oc, k5 = _ptr(out_counts)
        rp, k6 = _ptr(gr)
        self._ck(self._L.mp3d_batch_limit(self._h, sp if ss else None, ss, cp, n, gp, op, int(bool(f32)), stride, oc, rp,
                                          _pack_flags(flush), _stream(stream)))
        return out, out_counts, gr

    def decode_limited(self, frames, offsets, sizes, frames_per_stream, gain=None, out=None, counts=None, gr=None,
                       infos=None, f32=True, flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        samples times gain through the limiter (mp3d_batch_decode_limited).
        stride defaults to out's, else to the bound that cannot overflow.
        flush and gapless as in decode_packed; the flush also ends the
        limiter.  Returns (out, counts, gr, infos)."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        out, counts, gain, gr, stride = self._limit_args(
            n, out, counts, gain, gr, f32, stride, lambda hz: limiter_max_samples(hz, packed_max_samples(hz, F)))
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        gp, k2 = _ptr(gain)
        op, k3 = _ptr(out)
        cp, k4 = _ptr(counts)
        rp, k5 = _ptr(gr)
        ip, k6 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_limited(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, gp, op,
                                                   int(bool(f32)), stride, cp, rp,
                                                   _pack_flags(flush, gapless), ip, _stream(stream)))
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

    def _eq_args(self, n, out, out_counts, stride, default_stride):
        hz, ch = getattr(self, "_out", (0, 0))
        if stride is None:  # (equaliser off: the call fails with MP3D_E_ARG)
            stride = int(out.shape[1]) if out is not None else default_stride(hz) if getattr(self, "_eq", 0) else 1
        stride = int(stride)
        if out is None:
            out = np.zeros((n, stride, ch), np.float32)
        if out_counts is None:
            out_counts = np.zeros(n, np.int32)
        return out, out_counts, stride

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
        n, ss = int(samples.shape[0]), int(samples.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        out, out_counts, stride = self._eq_args(n, out, out_counts, stride, lambda hz: ss)
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        op, k3 = _ptr(out)
        oc, k4 = _ptr(out_counts)
        self._ck(self._L.mp3d_batch_eq(self._h, sp if ss else None, ss, cp, n, op, stride, oc, _pack_flags(flush),
                                       _stream(stream)))
        return out, out_counts

    def decode_equalized(self, frames, offsets, sizes, frames_per_stream, out=None, counts=None, infos=None,
                         flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        samples through the equaliser (mp3d_batch_decode_equalized).  stride
        defaults to out's, else to the bound that cannot overflow.  flush and
        gapless as in decode_packed; the flush also restarts the equaliser.
        Returns (out, counts, infos)."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        out, counts, stride = self._eq_args(n, out, counts, stride, lambda hz: packed_max_samples(hz, F))
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        op, k2 = _ptr(out)
        cp, k3 = _ptr(counts)
        ip, k4 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_equalized(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, op, stride, cp,
                                                     _pack_flags(flush, gapless), ip, _stream(stream)))
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
            energy = [segment_threshold(getattr(self, "_out", (0, 0))[0], db)] * int(n)
        thr = np.ascontiguousarray(energy, np.uint64).reshape(-1)
        self._ck(self._L.mp3d_batch_set_segment_threshold(self._h, int(first), thr.size, thr.ctypes.data))

    def _segment_args(self, n, seg, seg_counts, stride, default_stride):
        hz, ch = getattr(self, "_out", (0, 0))
        if stride is None:  # (sink off: the call fails with MP3D_E_ARG)
            on = getattr(self, "_segments", None)
            stride = int(seg.shape[1]) if seg is not None else default_stride(hz, *on) if on else 1
        stride = int(stride)
        if seg is None:
            seg = np.zeros((n, stride, 2), np.int64)
        if seg_counts is None:
            seg_counts = np.zeros(n, np.int32)
        return seg, seg_counts, stride

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
        n, ss = int(samples.shape[0]), int(samples.shape[1])
        if not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, np.int32)
        seg, seg_counts, stride = self._segment_args(n, seg, seg_counts, stride,
                                                     lambda hz, p, sp: segment_max(hz, ss, p, sp))
        sp, k1 = _ptr(samples)
        cp, k2 = _ptr(counts)
        gp, k3 = _ptr(seg)
        gc, k4 = _ptr(seg_counts)
        self._ck(self._L.mp3d_batch_segments(self._h, sp if ss else None, ss, cp, n, gp, stride, gc, _pack_flags(flush),
                                             _stream(stream)))
        return seg, seg_counts

    def decode_segments(self, frames, offsets, sizes, frames_per_stream, seg=None, counts=None, infos=None,
                        flush=False, stride=None, stream=None, gapless=False):
        """Decode as decode_packed does (float32) and write every stream's
        segments (mp3d_batch_decode_segments).  stride defaults to seg's, else
        to the bound that cannot overflow.  flush and gapless as in
        decode_packed; the flush also ends the segments.  Returns (seg, counts,
        infos)."""
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        seg, counts, stride = self._segment_args(
            n, seg, counts, stride, lambda hz, p, sp: segment_max(hz, packed_max_samples(hz, F), p, sp))
        if infos is None:
            infos = np.zeros((n, F), FRAME_INFO_DT)
        fp, k1 = _ptr(frames)
        gp, k2 = _ptr(seg)
        cp, k3 = _ptr(counts)
        ip, k4 = _ptr(infos)
        self._ck(self._L.mp3d_batch_decode_segments(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F, gp, stride, cp,
                                                    _pack_flags(flush, gapless), ip, _stream(stream)))
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

        hz, ch = getattr(self, "_out", (0, 0))
        if getattr(self, "_segments", None) is None:
            raise MP3DError("long_segments needs set_segments")
        host = data.cpu().numpy().tobytes() if hasattr(data, "cpu") else bytes(data)
        cap = max(1, long_packed_bound(host, hz))
        out = torch.zeros((cap, ch), dtype=torch.float32, device="cuda:%d" % self.device)
        pcm, si, in_hz = self.decode_long_packed(data, hz, ch, segment_frames, out=out, gapless=gapless)
        n = int(pcm.shape[0])
        seg, cnt = self.segments(out[None, : max(n, 1)], [n], flush=True)
        return seg[0, : int(cnt[0])].copy(), pcm, si, in_hz

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
        if not (getattr(self, "_loud", False) and getattr(self, "_tp", False)):
            raise MP3DError("decode_normalized needs set_loudness and set_true_peak")
        if limit:
            if getattr(self, "_limit", None) is None:
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
        off, sz = self._geom(offsets, sizes)
        n, F = off.size, int(frames_per_stream)
        is_out = np.zeros((n, F, 2, 2, 576), np.int16)
        sf_out = np.zeros((n, F, 2, 2, 40), np.uint8)
        fp, k1 = _ptr(frames)
        self._ck(self._L.mp3d_batch_huffman_only(self._h, fp, off.ctypes.data, sz.ctypes.data, n, F,
                                             is_out.ctypes.data, sf_out.ctypes.data, None))
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


EQ_MAX_BANDS = 10  # MP3D_EQ_MAX_BANDS
EQ_PEAK, EQ_LOW_SHELF, EQ_HIGH_SHELF, EQ_HIGH_PASS, EQ_LOW_PASS = range(5)  # MP3D_EQ_*
EQ_BAND_DT = np.dtype([("type", np.int32), ("f0_hz", np.float64), ("gain_db", np.float64), ("q", np.float64)],
                      align=True)  # mp3d_eq_band


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
