"""The C ABI of include/mp3d.h as ctypes sees it: the structs and constants,
one table of every export's signature, and the loader that binds a build of
the library to it.  mp3_amd/__init__.py re-exports all of it."""
import contextlib
import ctypes
import os
import pathlib

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ["MP3D_LIB"]) if os.environ.get("MP3D_LIB") else _HERE / "libmp3d.so"


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

OPT_CRC_CHECK = 1  # MP3D_OPT_CRC_CHECK: drop frames whose CRC-16 mismatches
LONG_GAPLESS = 1  # MP3D_LONG_GAPLESS: apply the LAME tag's trim inside decode_long_packed
PACK_FLUSH = 1  # MP3D_PACK_FLUSH: feed zeros after the call's frames, then restart the resamplers
PACK_GAPLESS = 2  # MP3D_PACK_GAPLESS: fix an unfixed sample window from the stream's LAME tag (decode_packed/_features)
WINDOW_NO_END = 2**63 - 1  # MP3D_WINDOW_NO_END: a sample window without an end
FEAT_LOG10 = 1  # MP3D_FEAT_LOG10: log10(max(mel, 1e-10)) instead of the mel energies
MP3D_FEAT_LOG10 = FEAT_LOG10
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
FRAME_F32, FRAME_LAST = 1, 2  # mp3d_decode_frame_ex flags
EQ_MAX_BANDS = 10  # MP3D_EQ_MAX_BANDS
EQ_PEAK, EQ_LOW_SHELF, EQ_HIGH_SHELF, EQ_HIGH_PASS, EQ_LOW_PASS = range(5)  # MP3D_EQ_*
EQ_BAND_DT = np.dtype([("type", np.int32), ("f0_hz", np.float64), ("gain_db", np.float64), ("q", np.float64)],
                      align=True)  # mp3d_eq_band
PITCH_FRAME_DT = np.dtype([("f0_hz", np.float32), ("periodicity", np.float32), ("lag", np.int32),
                           ("shift", np.int32)])  # mp3d_pitch_frame


def _abi():
    """name -> (restype, argtypes) of every export, in the header's terms:
    a pointer the wrappers fill from an array or a tensor is a void pointer,
    one they pass by reference is typed, a byte string is c_char_p."""
    i, ll, dbl, sz, vp, s = (ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p,
                             ctypes.c_char_p)
    P = ctypes.POINTER
    ip, finfo, sinfo = P(i), P(FrameInfo), P(StreamInfo)
    dec = [vp, vp, vp, vp, i, i]  # handle, frames, offsets, sizes, n_streams, frames_per_stream
    one = [vp, vp, ll, vp, i]  # handle, samples, sample_stride, counts, n_streams
    tail = [i, vp, vp]  # flags, infos, hip_stream
    time = (i, [vp, vp])  # handle, float *us
    return {
        "mp3d_dec_create": (i, [P(vp)]),
        "mp3d_dec_create_on": (i, [i, P(vp)]),
        "mp3d_dec_destroy": (None, [vp]),
        "mp3d_dec_reset": (None, [vp]),
        "mp3d_decode_frame": (i, [vp, s, sz, vp, finfo]),
        "mp3d_decode_frame_f32": (i, [vp, s, sz, vp, finfo]),
        "mp3d_batch_decode_f32": (i, dec + [vp, vp, vp]),
        "mp3d_batch_create": (i, [i, i, i, P(vp)]),
        "mp3d_batch_destroy": (None, [vp]),
        "mp3d_batch_reset": (i, [vp]),
        "mp3d_batch_decode": (i, dec + [vp, vp, vp]),
        "mp3d_batch_sync": (i, [vp]),
        "mp3d_batch_huffman_only": (i, dec + [vp, vp, vp]),
        "mp3d_batch_synth_only": (i, [vp, vp, vp, vp, i, i, i, i, vp, vp]),
        "mp3d_strerror": (s, [i]),
        "mp3d_last_hip_error": (i, []),
        "mp3d_abi_version": (i, []),
        "mp3d_batch_set_timing": (i, [vp, i]),
        "mp3d_batch_kernel_times": (i, [vp, vp]),
        "mp3d_batch_stream_info": (i, [vp, i, vp]),
        "mp3d_dec_stream_info": (i, [vp, sinfo]),
        "mp3d_batch_decode_long": (i, [vp, vp, sz, i, vp, i, ll, vp, P(ll), sinfo]),
        "mp3d_long_plan": (i, [s, sz, i, ll, vp, vp, P(ll), ip]),
        "mp3d_batch_set_options": (i, [vp, i]),
        "mp3d_dec_set_options": (i, [vp, i]),
        "mp3d_decode_frame_ex": (i, [vp, s, sz, vp, i, finfo]),
        "mp3d_state_bytes": (sz, []),
        "mp3d_batch_get_state": (i, [vp, i, i, vp]),
        "mp3d_batch_set_state": (i, [vp, i, i, vp]),
        "mp3d_dec_get_state": (i, [vp, vp]),
        "mp3d_dec_set_state": (i, [vp, vp]),
        "mp3d_resample_filter": (ll, [i, i, ip, ip, ip, vp, sz]),
        "mp3d_batch_set_output": (i, [vp, i, i]),
        "mp3d_packed_max_samples": (ll, [i, i, i]),
        "mp3d_batch_decode_packed": (i, dec + [vp, i, ll, vp] + tail),
        "mp3d_batch_resample_time": time,
        "mp3d_batch_decode_long_packed": (i, [vp, vp, sz, i, i, i, vp, i, ll, P(ll), i, sinfo, ip]),
        "mp3d_long_packed_bound": (ll, [s, sz, i]),
        "mp3d_mel_filterbank": (ll, [i, vp, sz]),
        "mp3d_feat_max_frames": (ll, [i, i]),
        "mp3d_batch_set_features": (i, [vp, i, i]),
        "mp3d_batch_decode_features": (i, dec + [vp, ll, vp] + tail),
        "mp3d_batch_features": (i, one + [vp, ll, vp, i, vp]),
        "mp3d_batch_feature_time": time,
        "mp3d_batch_set_window": (i, [vp, i, i, vp, vp]),
        "mp3d_batch_sink_window": (i, [vp, i, i, vp, vp, vp]),
        "mp3d_loudness_filter": (ll, [i, vp, sz]),
        "mp3d_loud_max_blocks": (ll, [i, i, i]),
        "mp3d_batch_set_loudness": (i, [vp, i]),
        "mp3d_batch_loudness": (i, one + [vp, ll, vp, vp, i, vp]),
        "mp3d_batch_decode_loudness": (i, dec + [vp, ll, vp, vp] + tail),
        "mp3d_loudness_integrated": (i, [vp, ll, P(dbl)]),
        "mp3d_batch_loudness_integrated": (i, one + [vp, vp]),
        "mp3d_batch_loudness_time": time,
        "mp3d_truepeak_filter": (ll, [vp, sz]),
        "mp3d_batch_set_true_peak": (i, [vp, i]),
        "mp3d_batch_true_peak": (i, one + [vp, i, vp]),
        "mp3d_batch_decode_measure": (i, dec + [vp, ll, vp, vp, vp] + tail),
        "mp3d_batch_normalize_gain": (i, [vp, vp, vp, i, dbl, dbl, vp, vp]),
        "mp3d_batch_apply_gain": (i, one + [vp, vp, i, vp]),
        "mp3d_batch_true_peak_time": time,
        "mp3d_stretch_window": (ll, [i, vp, sz]),
        "mp3d_stretch_max_samples": (ll, [i, ll, i, i]),
        "mp3d_batch_set_stretch": (i, [vp, i]),
        "mp3d_batch_set_tempo": (i, [vp, i, i, vp, vp]),
        "mp3d_batch_stretch": (i, one + [vp, ll, vp, i, vp]),
        "mp3d_batch_decode_stretched": (i, dec + [vp, ll, vp] + tail),
        "mp3d_batch_stretch_time": time,
        "mp3d_limiter_lookahead": (ll, [i]),
        "mp3d_limiter_max_samples": (ll, [i, ll]),
        "mp3d_batch_set_limiter": (i, [vp, i, dbl]),
        "mp3d_batch_limit": (i, one + [vp, vp, i, ll, vp, vp, i, vp]),
        "mp3d_batch_decode_limited": (i, dec + [vp, vp, i, ll, vp, vp] + tail),
        "mp3d_batch_limiter_time": time,
        "mp3d_segment_threshold": (ll, [i, dbl]),
        "mp3d_segment_max": (ll, [i, ll, i, i]),
        "mp3d_batch_set_segments": (i, [vp, i, i, i, i]),
        "mp3d_batch_set_segment_threshold": (i, [vp, i, i, vp]),
        "mp3d_batch_segments": (i, one + [vp, ll, vp, i, vp]),
        "mp3d_batch_decode_segments": (i, dec + [vp, ll, vp] + tail),
        "mp3d_batch_segment_time": time,
        "mp3d_eq_design": (ll, [i, vp, i, dbl, vp, sz]),
        "mp3d_batch_set_eq": (i, [vp, vp, i, dbl]),
        "mp3d_batch_eq": (i, one + [vp, ll, vp, i, vp]),
        "mp3d_batch_decode_equalized": (i, dec + [vp, ll, vp] + tail),
        "mp3d_batch_eq_time": time,
        "mp3d_pitch_span": (ll, [i, i, i, ip, ip]),
        "mp3d_pitch_max_frames": (ll, [i, ll, i]),
        "mp3d_batch_set_pitch": (i, [vp, i, i, i, i]),
        "mp3d_batch_pitch": (i, one + [vp, ll, vp, i, vp]),
        "mp3d_batch_decode_pitch": (i, dec + [vp, ll, vp] + tail),
        "mp3d_batch_pitch_time": time,
    }


ABI = _abi()
EXPORTS = list(ABI)  # what include/mp3d.h declares (tests/test_abi.py)
# libmp3d_wglds.so only (tests/test_gpu_wglds.py): not part of the header
DEBUG_ABI = {"mp3d_debug_wglds_probe": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int])}

_lib = None


class MP3DError(RuntimeError):
    pass


def _bind(L):
    """Result and argument types of every export this build has (an older
    build loaded for an A/B lacks the later sinks; only the debug build has
    the probe)."""
    for table in (ABI, DEBUG_ABI):
        for name, (restype, argtypes) in table.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, list(argtypes)
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
