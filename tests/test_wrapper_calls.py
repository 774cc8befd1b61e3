"""No GPU: what BatchDecoder hands to the library, call by call.

A recording stand-in takes the library's place on a handle-less wrapper (as
Refuses does in test_packed_window_host.py): every export returns 0 and keeps
(name, args).  The tests pin, for every method that calls the library on
small host arrays (n = 2, F = 1, sample_stride 0 and 5), the export called,
the argument count (the loaded build's argtypes), the scalars (n, F, strides,
flags, the f32 flag), the pointers, and the shape and dtype of every result
the wrapper allocates, with the sinks never set, off and on.  The default
strides are the host-only exports' own bounds."""
import collections
import ctypes
import itertools

import numpy as np
import pytest

import mp3_amd as M

N, F, HZ, CH = 2, 1, 16000, 1  # (the feature sink needs 16 kHz mono)
FRAMES = np.zeros(16, np.uint8)
OFF = np.array([0, 8], np.uint64)  # already of the wrapper's types: it passes them on as they are
SZ = np.array([8, 8], np.uint32)
COUNTS = np.array([3, 5], np.int32)
HOP = (HZ + 5) // 10  # a loudness block's hop in samples
MODES = ("fresh", "off", "on")  # nothing set; set_output alone; the sink on
FLAGS = list(itertools.product((False, True), repeat=2))

# the arguments of the exports with a shared head or tail, by name
DEC = "h frames off sz n F "
ONE = "h samples ss counts n "
LAYOUT = {k: v.split() for k, v in {
    "mp3d_batch_decode": DEC + "out infos stream",
    "mp3d_batch_decode_f32": DEC + "out infos stream",
    "mp3d_batch_huffman_only": DEC + "is_out sf_out stream",
    "mp3d_batch_decode_packed": DEC + "out f32 stride ocounts flags infos stream",
    "mp3d_batch_decode_features": DEC + "out stride ocounts flags infos stream",
    "mp3d_batch_decode_loudness": DEC + "out stride ocounts peak flags infos stream",
    "mp3d_batch_decode_measure": DEC + "out stride ocounts peak tpeak flags infos stream",
    "mp3d_batch_decode_stretched": DEC + "out stride ocounts flags infos stream",
    "mp3d_batch_decode_limited": DEC + "gain out f32 stride ocounts gr flags infos stream",
    "mp3d_batch_decode_equalized": DEC + "out stride ocounts flags infos stream",
    "mp3d_batch_decode_segments": DEC + "out stride ocounts flags infos stream",
    "mp3d_batch_features": ONE + "out stride ocounts flags stream",
    "mp3d_batch_loudness": ONE + "out stride ocounts peak flags stream",
    "mp3d_batch_true_peak": ONE + "tpeak flags stream",
    "mp3d_batch_stretch": ONE + "out stride ocounts flags stream",
    "mp3d_batch_limit": ONE + "gain out f32 stride ocounts gr flags stream",
    "mp3d_batch_eq": ONE + "out stride ocounts flags stream",
    "mp3d_batch_segments": ONE + "out stride ocounts flags stream",
    "mp3d_batch_apply_gain": ONE + "gain out f32 stream",
    "mp3d_batch_loudness_integrated": ONE + "lufs stream",
    "mp3d_batch_normalize_gain": "h lufs tpeak n target max_dbtp gain stream",
}.items()}


class Records:
    """Stands in for the library: every export returns 0 and is recorded.
    peek[name] = [(argument index, dtype, count)]: arrays to copy while the
    call runs (the wrapper's own temporaries are gone after it)."""

    def __init__(self):
        self.calls, self.peek, self.peeked = [], {}, []

    def __getattr__(self, name):
        if not name.startswith("mp3d_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            for k, dt, cnt in self.peek.get(name, ()):
                raw = (ctypes.c_char * (cnt * np.dtype(dt).itemsize)).from_address(args[k])
                self.peeked.append(np.frombuffer(raw, dt).copy())
            return 0
        return call


def wrapper():
    dec = M.BatchDecoder.__new__(M.BatchDecoder)
    dec._L, dec._h, dec.max_streams, dec.max_frames, dec.device = Records(), ctypes.c_void_p(0x1000), 4, 2, 0
    return dec


def called(dec, *names):
    """The arguments of the calls made since the last look, which must be
    those of `names`: each as many as the loaded build's export takes, each
    one its ctypes type accepts, the handle first.  One name: its arguments,
    by name where the export has a LAYOUT."""
    calls = list(dec._L.calls)
    dec._L.calls.clear()
    assert [c[0] for c in calls] == list(names)
    res = []
    for name, args in calls:
        types = getattr(M.lib(), name).argtypes
        assert len(args) == len(types), name
        for t, a in zip(types, args):
            t.from_param(a)
        assert args[0] is dec._h
        if name in LAYOUT:
            assert len(LAYOUT[name]) == len(args), name
            args = dict(zip(LAYOUT[name], args))
        res.append(args)
    return res[0] if len(names) == 1 else res


def host(x, shape, dtype):
    """x is a host array of this shape and dtype; returns its address."""
    assert isinstance(x, np.ndarray) and x.shape == tuple(shape) and x.dtype == np.dtype(dtype), (x.shape, x.dtype)
    return x.ctypes.data


def stream_of(a):
    return a.value if a is not None else None


def decode_head(a, infos):
    assert (a["frames"], a["off"], a["sz"]) == (FRAMES.ctypes.data, OFF.ctypes.data, SZ.ctypes.data)
    assert (a["n"], a["F"]) == (N, F) and type(a["n"]) is int and type(a["F"]) is int
    assert a["infos"] == host(infos, (N, F), M.FRAME_INFO_DT)


def stage_head(a, smp, ss):
    assert a["samples"] == (smp.ctypes.data if ss else None)
    assert (a["ss"], a["counts"], a["n"]) == (ss, COUNTS.ctypes.data, N)


Sink = collections.namedtuple("Sink", "name on decode alone out cnt tail dtype dbound abound")


def packed_bound(hz):
    return M.packed_max_samples(hz, F)


SINKS = [
    Sink("packed", lambda d: None, "decode_packed", None, "out", None, lambda ch, on: (ch,), np.float32,
         packed_bound, None),
    Sink("features", lambda d: d.set_features(8), "decode_features", "features", "feat", "feat_counts",
         lambda ch, on: (8 if on else 1,), np.float32,
         lambda hz: M.feat_max_frames(F), lambda hz, ss: (ss + 200 + 159) // 160 + 1),
    Sink("loudness", lambda d: d.set_loudness(), "decode_loudness", "loudness", "blocks", "block_counts",
         lambda ch, on: (), np.float32,
         lambda hz: M.loud_max_blocks(hz, F), lambda hz, ss: (HOP - 1 + ss) // HOP),
    Sink("measure", lambda d: (d.set_loudness(), d.set_true_peak()), "decode_measure", None, "blocks", None,
         lambda ch, on: (), np.float32, lambda hz: M.loud_max_blocks(hz, F), None),
    Sink("stretch", lambda d: d.set_stretch(), "decode_stretched", "stretch", "out", "out_counts",
         lambda ch, on: (ch,), np.float32,
         lambda hz: M.stretch_max_samples(hz, packed_bound(hz), 1, 2),
         lambda hz, ss: M.stretch_max_samples(hz, ss, 1, 2)),
    Sink("limiter", lambda d: d.set_limiter(True, -2.0), "decode_limited", "limit", "out", "out_counts",
         lambda ch, on: (ch,), np.float32,
         lambda hz: M.limiter_max_samples(hz, packed_bound(hz)), lambda hz, ss: M.limiter_max_samples(hz, ss)),
    Sink("eq", lambda d: d.set_eq([(M.EQ_PEAK, 1000.0, 3.0, 1.0)]), "decode_equalized", "eq", "out", "out_counts",
         lambda ch, on: (ch,), np.float32, packed_bound, lambda hz, ss: ss),
    Sink("segments", lambda d: d.set_segments(True, min_pause_ms=200, min_speech_ms=80), "decode_segments", "segments",
         "seg", "seg_counts", lambda ch, on: (2,), np.int64,
         lambda hz: M.segment_max(hz, packed_bound(hz), 20, 8), lambda hz, ss: M.segment_max(hz, ss, 20, 8)),
]
ALONE = [s for s in SINKS if s.alone]
by_name = pytest.mark.parametrize("sink", SINKS, ids=lambda s: s.name)
alone_by_name = pytest.mark.parametrize("sink", ALONE, ids=lambda s: s.name)


def make(sink, mode):
    """(wrapper, hz, channels, whether the sink is on)"""
    dec = wrapper()
    if mode == "fresh":
        return dec, 0, 0, False
    dec.set_output(HZ, CH)
    if mode == "on":
        sink.on(dec)
    dec._L.calls.clear()
    return dec, HZ, CH, mode == "on" or sink.name == "packed"


def samples(sink, ss, ch):
    return np.zeros((N, ss) if sink.name == "features" else (N, ss, max(ch, 1)), np.float32)


def extras(sink, a, r):
    """the results next to out and its counts, by sink"""
    if sink.name in ("loudness", "measure"):
        assert a["peak"] == host(r[2], (N,), np.float32) and not r[2].any()
    if sink.name == "measure":
        assert a["tpeak"] == host(r[3], (N,), np.float32) and not r[3].any()
    if sink.name == "limiter":
        assert a["gr"] == host(r[2], (N,), np.float32) and (r[2] == 1).all()
        assert a["gain"] is None and a["f32"] == 1
    if sink.name == "packed":
        assert a["f32"] == 1


@by_name
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("flush,gapless", FLAGS)
def test_decode_defaults(sink, mode, flush, gapless):
    dec, hz, ch, on = make(sink, mode)
    r = getattr(dec, sink.decode)(FRAMES, OFF, SZ, F, flush=flush, gapless=gapless)
    a = called(dec, "mp3d_batch_" + sink.decode)
    decode_head(a, r[-1])
    stride = sink.dbound(hz) if on else 1
    assert a["stride"] == stride and type(a["stride"]) is int
    assert a["out"] == host(r[0], (N, stride) + sink.tail(ch, on), sink.dtype) and not r[0].any()
    assert a["ocounts"] == host(r[1], (N,), np.int32) and not r[1].any()
    assert a["flags"] == (M.PACK_FLUSH if flush else 0) | (M.PACK_GAPLESS if gapless else 0)
    assert a["stream"] is None
    extras(sink, a, r)


@alone_by_name
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ss", (0, 5))
@pytest.mark.parametrize("flush", (False, True))
def test_stage_alone_defaults(sink, mode, ss, flush):
    dec, hz, ch, on = make(sink, mode)
    smp = samples(sink, ss, ch)
    r = getattr(dec, sink.alone)(smp, COUNTS, flush=flush)
    a = called(dec, "mp3d_batch_" + sink.alone)
    stage_head(a, smp, ss)
    stride = sink.abound(hz, ss) if on else 1
    assert a["stride"] == stride and type(a["stride"]) is int
    assert a["out"] == host(r[0], (N, stride) + sink.tail(ch, on), sink.dtype)
    assert a["ocounts"] == host(r[1], (N,), np.int32)
    assert a["flags"] == (M.PACK_FLUSH if flush else 0) and a["stream"] is None
    extras(sink, a, r)


@by_name
def test_decode_given_buffers(sink):
    """out, counts and infos of the caller's go through as they are; the
    stride is out's; a stream handle arrives as a pointer."""
    dec, hz, ch, on = make(sink, "on")
    out = np.zeros((N, 7) + sink.tail(ch, on), sink.dtype)
    counts, infos = np.zeros(N, np.int32), np.zeros((N, F), M.FRAME_INFO_DT)
    r = getattr(dec, sink.decode)(FRAMES, OFF, SZ, F, **{sink.out: out}, counts=counts, infos=infos, stream=77)
    a = called(dec, "mp3d_batch_" + sink.decode)
    decode_head(a, infos)
    assert r[0] is out and r[1] is counts and r[-1] is infos
    assert (a["out"], a["stride"], a["ocounts"]) == (out.ctypes.data, 7, counts.ctypes.data)
    assert stream_of(a["stream"]) == 77


@alone_by_name
def test_stage_alone_given_buffers(sink):
    dec, hz, ch, on = make(sink, "on")
    smp = samples(sink, 5, ch)
    out, oc = np.zeros((N, 7) + sink.tail(ch, on), sink.dtype), np.zeros(N, np.int32)
    r = getattr(dec, sink.alone)(smp, COUNTS, **{sink.out: out, sink.cnt: oc}, stream=77)
    a = called(dec, "mp3d_batch_" + sink.alone)
    stage_head(a, smp, 5)
    assert r[0] is out and r[1] is oc
    assert (a["out"], a["stride"], a["ocounts"]) == (out.ctypes.data, 7, oc.ctypes.data)
    assert stream_of(a["stream"]) == 77


@by_name
@pytest.mark.parametrize("mode", MODES)
def test_given_stride_sizes_the_default_out(sink, mode):
    dec, hz, ch, on = make(sink, mode)
    r = getattr(dec, sink.decode)(FRAMES, OFF, SZ, F, stride=np.int64(3))
    a = called(dec, "mp3d_batch_" + sink.decode)
    assert a["stride"] == 3 and type(a["stride"]) is int
    assert a["out"] == host(r[0], (N, 3) + sink.tail(ch, on), sink.dtype)
    if sink.alone:
        r = getattr(dec, sink.alone)(samples(sink, 5, ch), COUNTS, stride=3)
        a = called(dec, "mp3d_batch_" + sink.alone)
        assert a["stride"] == 3 and a["out"] == host(r[0], (N, 3) + sink.tail(ch, on), sink.dtype)


def test_set_output_turns_every_sink_off():
    dec = wrapper()
    dec.set_output(HZ, CH)
    for sink in SINKS:
        sink.on(dec)
    assert dec._out == (HZ, CH) and dec._segments == (20, 8)
    dec.set_output(HZ, CH)
    assert dec._out == (HZ, CH) and dec._segments is None
    dec._L.calls.clear()
    for sink in SINKS[1:]:
        r = getattr(dec, sink.decode)(FRAMES, OFF, SZ, F)
        a = called(dec, "mp3d_batch_" + sink.decode)
        assert a["stride"] == 1 and r[0].shape == (N, 1) + sink.tail(CH, False), sink.name
    dec.set_output(0, 0)
    assert dec._out == (0, 0)
    out, counts, infos = dec.decode_packed(FRAMES, OFF, SZ, F)
    assert out.shape == (N, 1, 0) and called(dec, "mp3d_batch_set_output", "mp3d_batch_decode_packed")[1]["stride"] == 1


def test_sink_switches():
    """every set_* call: its export and scalars, and what it leaves behind"""
    dec = wrapper()
    dec.set_output(HZ, 2)
    assert called(dec, "mp3d_batch_set_output")[1:] == (HZ, 2) and dec._out == (HZ, 2)
    dec.set_features(8)
    assert called(dec, "mp3d_batch_set_features")[1:] == (8, M.FEAT_LOG10)
    dec.set_features(np.int64(40), log10=False)
    a = called(dec, "mp3d_batch_set_features")
    assert a[1:] == (40, 0) and type(a[1]) is int
    for name in ("loudness", "true_peak", "stretch"):
        getattr(dec, "set_" + name)()
        assert called(dec, "mp3d_batch_set_" + name)[1:] == (1,)
        getattr(dec, "set_" + name)(0)
        assert called(dec, "mp3d_batch_set_" + name)[1:] == (0,)
    dec.set_limiter(True, -3)
    a = called(dec, "mp3d_batch_set_limiter")
    assert a[1:] == (1, -3.0) and type(a[2]) is float
    dec.set_limiter(False)
    assert called(dec, "mp3d_batch_set_limiter")[1:] == (0, -1.0)
    dec.set_segments()
    assert called(dec, "mp3d_batch_set_segments")[1:] == (1, 30, 10, 5) and dec._segments == (30, 10)
    dec._L.peek["mp3d_batch_set_segment_threshold"] = [(3, np.uint64, 4)]
    dec.set_segments(True, threshold_db=-30.0, min_pause_ms=204, min_speech_ms=96, pad_ms=0)
    a, b = called(dec, "mp3d_batch_set_segments", "mp3d_batch_set_segment_threshold")
    assert a[1:] == (1, 20, 10, 0) and dec._segments == (20, 10)
    assert b[1:3] == (0, 4) and (dec._L.peeked.pop() == M.segment_threshold(HZ, -30.0)).all()
    dec.set_segments(False, threshold_db=-30.0)
    assert called(dec, "mp3d_batch_set_segments")[1:] == (0, 30, 10, 5) and dec._segments is None
    dec._L.peek["mp3d_batch_set_eq"] = [(1, M.EQ_BAND_DT, 2)]
    dec.set_eq([(M.EQ_LOW_SHELF, 100, 3, 0.7), (M.EQ_PEAK, 1000.0, -2.0, 1.0)], preamp_db=-1)
    a = called(dec, "mp3d_batch_set_eq")
    assert a[2:] == (2, -1.0) and type(a[3]) is float
    assert dec._L.peeked.pop().tolist() == [(M.EQ_LOW_SHELF, 100.0, 3.0, 0.7), (M.EQ_PEAK, 1000.0, -2.0, 1.0)]
    del dec._L.peek["mp3d_batch_set_eq"]
    for off in (None, []):
        dec.set_eq(off)
        assert called(dec, "mp3d_batch_set_eq")[1:] == (None, 0, 0.0)


def test_segment_threshold_and_tempo():
    dec = wrapper()
    dec.set_output(HZ, CH)
    dec._L.calls.clear()
    dec._L.peek["mp3d_batch_set_segment_threshold"] = [(3, np.uint64, 2)]
    dec.set_segment_threshold(energy=[7, 9], first=1)
    assert called(dec, "mp3d_batch_set_segment_threshold")[1:3] == (1, 2) and dec._L.peeked.pop().tolist() == [7, 9]
    dec.set_segment_threshold(db=-20.0, first=2, n=2)
    assert called(dec, "mp3d_batch_set_segment_threshold")[1:3] == (2, 2)
    assert dec._L.peeked.pop().tolist() == [M.segment_threshold(HZ, -20.0)] * 2
    for bad in ({}, {"db": -20.0, "energy": 5}):
        with pytest.raises(ValueError):
            dec.set_segment_threshold(**bad)
    dec._L.peek["mp3d_batch_set_tempo"] = [(3, np.int32, 2), (4, np.int32, 2)]
    dec.set_tempo([3, 1], [2, 2], first=1)
    assert called(dec, "mp3d_batch_set_tempo")[1:3] == (1, 2)
    assert [p.tolist() for p in dec._L.peeked] == [[3, 1], [2, 2]]
    with pytest.raises(ValueError):
        dec.set_tempo([3, 1], [2])
    assert not dec._L.calls


@pytest.mark.parametrize("f32", (False, True))
def test_decode(f32):
    dec = wrapper()
    pcm, infos = dec.decode(FRAMES, OFF, SZ, F, f32=f32)
    a = called(dec, "mp3d_batch_decode_f32" if f32 else "mp3d_batch_decode")
    decode_head(a, infos)
    assert a["out"] == host(pcm, (N, F, 2304), np.float32 if f32 else np.int16) and a["stream"] is None
    given = np.zeros((N, F, 2304), np.int16), np.zeros((N, F), M.FRAME_INFO_DT)
    assert dec.decode(FRAMES, OFF, SZ, F, pcm=given[0], infos=given[1], stream=5) == given
    a = called(dec, "mp3d_batch_decode")
    assert (a["out"], a["infos"], stream_of(a["stream"])) == (given[0].ctypes.data, given[1].ctypes.data, 5)


def test_geometry_is_coerced_and_checked():
    dec = wrapper()
    dec._L.peek["mp3d_batch_decode_packed"] = [(2, np.uint64, 2), (3, np.uint32, 2)]
    dec.decode_packed(FRAMES.tobytes(), [0, 8], (8, 8), np.int64(1))
    a = called(dec, "mp3d_batch_decode_packed")
    assert [p.tolist() for p in dec._L.peeked] == [[0, 8], [8, 8]]
    assert (a["n"], a["F"]) == (N, F) and type(a["F"]) is int
    for fn in (dec.decode, dec.decode_packed, dec.decode_features, dec.decode_loudness, dec.decode_measure,
               dec.decode_stretched, dec.decode_limited, dec.decode_equalized, dec.decode_segments, dec.huffman_only):
        with pytest.raises(ValueError):
            fn(FRAMES, [0, 8], [8], F)
    assert not dec._L.calls


def test_staged_entry_points():
    dec = wrapper()
    is_out, sf_out = dec.huffman_only(FRAMES, OFF, SZ, F)
    a = called(dec, "mp3d_batch_huffman_only")
    assert (a["frames"], a["off"], a["sz"]) == (FRAMES.ctypes.data, OFF.ctypes.data, SZ.ctypes.data)
    assert (a["n"], a["F"]) == (N, F)
    assert a["is_out"] == host(is_out, (N, F, 2, 2, 576), np.int16)
    assert a["sf_out"] == host(sf_out, (N, F, 2, 2, 40), np.uint8) and a["stream"] is None
    xr = np.zeros((N, F, 2, 2, 576), np.float32)
    bt, mixed = np.zeros((N, F, 2, 2), np.uint8), np.zeros((N, F, 2, 2), np.uint8)
    pcm = dec.synth_only(xr, bt, mixed, 2, 44100, stream=9)
    a = called(dec, "mp3d_batch_synth_only")
    assert a[1:9] == (xr.ctypes.data, bt.ctypes.data, mixed.ctypes.data, N, F, 2, 44100,
                      host(pcm, (N, F, 2304), np.int16)) and a[9].value == 9


@pytest.mark.parametrize("f32", (False, True))
def test_f32_flag_picks_the_dtype(f32):
    dt = np.float32 if f32 else np.int16
    dec, hz, ch, on = make(SINKS[5], "on")
    stride = packed_bound(hz)
    out = dec.decode_packed(FRAMES, OFF, SZ, F, f32=f32)[0]
    a = called(dec, "mp3d_batch_decode_packed")
    assert a["f32"] == int(f32) and a["out"] == host(out, (N, stride, ch), dt)
    out = dec.decode_limited(FRAMES, OFF, SZ, F, f32=f32)[0]
    a = called(dec, "mp3d_batch_decode_limited")
    assert a["f32"] == int(f32) and a["out"] == host(out, (N, M.limiter_max_samples(hz, stride), ch), dt)
    smp = samples(SINKS[5], 5, ch)
    out = dec.limit(smp, COUNTS, f32=f32)[0]
    a = called(dec, "mp3d_batch_limit")
    assert a["f32"] == int(f32) and a["out"] == host(out, (N, M.limiter_max_samples(hz, 5), ch), dt)
    out = dec.apply_gain(smp, COUNTS, np.ones(N, np.float32), f32=f32)
    a = called(dec, "mp3d_batch_apply_gain")
    assert a["f32"] == int(f32) and a["out"] == host(out, smp.shape, dt)


def test_limiter_gain_and_gr():
    dec, hz, ch, on = make(SINKS[5], "on")
    gain, gr = np.array([0.5, 2.0], np.float32), np.zeros(N, np.float32)
    smp = samples(SINKS[5], 5, ch)
    assert dec.limit(smp, COUNTS, gain, gr=gr)[2] is gr
    a = called(dec, "mp3d_batch_limit")
    assert (a["gain"], a["gr"]) == (gain.ctypes.data, gr.ctypes.data)
    assert dec.decode_limited(FRAMES, OFF, SZ, F, gain=gain, gr=gr)[2] is gr
    a = called(dec, "mp3d_batch_decode_limited")
    assert (a["gain"], a["gr"]) == (gain.ctypes.data, gr.ctypes.data)
    dec._L.peek = {"mp3d_batch_limit": [(5, np.float32, N)], "mp3d_batch_decode_limited": [(6, np.float32, N)]}
    dec.limit(smp, COUNTS, [0.5, 2])
    dec.decode_limited(FRAMES, OFF, SZ, F, gain=[0.25, 4])
    assert [p.tolist() for p in dec._L.peeked] == [[0.5, 2.0], [0.25, 4.0]]


@pytest.mark.parametrize("ss", (0, 5))
@pytest.mark.parametrize("flush", (False, True))
def test_true_peak(ss, flush):
    dec = wrapper()
    smp = np.zeros((N, ss, CH), np.float32)
    tpeak = dec.true_peak(smp, COUNTS, flush=flush)
    a = called(dec, "mp3d_batch_true_peak")
    stage_head(a, smp, ss)
    assert a["tpeak"] == host(tpeak, (N,), np.float32) and not tpeak.any()
    assert a["flags"] == (M.PACK_FLUSH if flush else 0) and a["stream"] is None
    wide, given = np.zeros((N, 9, CH), np.float32), np.zeros(N, np.float32)
    assert dec.true_peak(wide, COUNTS, tpeak=given, stride=ss, stream=3) is given  # the stride in place of shape[1]
    a = called(dec, "mp3d_batch_true_peak")
    stage_head(a, wide, ss)
    assert (a["tpeak"], stream_of(a["stream"])) == (given.ctypes.data, 3)


@pytest.mark.parametrize("ss", (0, 5))
def test_gain_stages(ss):
    dec = wrapper()
    blocks = np.zeros((N, ss), np.float32)
    lufs = dec.integrated_lufs(blocks, COUNTS)
    a = called(dec, "mp3d_batch_loudness_integrated")
    stage_head(a, blocks, ss)
    assert a["lufs"] == host(lufs, (N,), np.float32) and a["stream"] is None
    assert dec.integrated_lufs(blocks, COUNTS, lufs=lufs, stream=4) is lufs
    assert stream_of(called(dec, "mp3d_batch_loudness_integrated")["stream"]) == 4

    tp = np.ones(N, np.float32)
    gain = dec.normalize_gain(lufs, tp)
    a = called(dec, "mp3d_batch_normalize_gain")
    assert (a["lufs"], a["tpeak"], a["n"]) == (lufs.ctypes.data, tp.ctypes.data, N)
    assert (a["target"], a["max_dbtp"]) == (-23.0, -1.0) and a["gain"] == host(gain, (N,), np.float32)
    assert dec.normalize_gain(lufs, None, target=-16, max_dbtp=-2, gain=gain, stream=4) is gain
    a = called(dec, "mp3d_batch_normalize_gain")
    assert (a["tpeak"], a["target"], a["max_dbtp"]) == (None, -16.0, -2.0)
    assert type(a["target"]) is float and stream_of(a["stream"]) == 4

    smp = np.zeros((N, ss, 2), np.float32)
    out = dec.apply_gain(smp, COUNTS, gain)
    a = called(dec, "mp3d_batch_apply_gain")
    stage_head(a, smp, ss)
    assert (a["gain"], a["f32"]) == (gain.ctypes.data, 1) and a["out"] == host(out, smp.shape, np.float32)
    assert dec.apply_gain(smp, COUNTS, gain, out=smp) is smp
    assert called(dec, "mp3d_batch_apply_gain")["out"] == smp.ctypes.data


def test_list_arguments_are_coerced():
    dec = wrapper()
    smp = np.zeros((N, 5, CH), np.float32)
    dec._L.peek = {"mp3d_batch_true_peak": [(3, np.int32, N)], "mp3d_batch_loudness_integrated": [(3, np.int32, N)],
                   "mp3d_batch_apply_gain": [(3, np.int32, N), (5, np.float32, N)],
                   "mp3d_batch_normalize_gain": [(1, np.float32, N), (2, np.float32, N)]}
    dec.true_peak(smp, [3, 5])
    dec.integrated_lufs(smp[:, :, 0].copy(), [1, 2])
    dec.apply_gain(smp, [3, 4], [0.5, 2])
    dec.normalize_gain([-20, -30.5], [1, 0.5])
    assert [p.tolist() for p in dec._L.peeked] == [[3, 5], [1, 2], [3, 4], [0.5, 2.0], [-20.0, -30.5], [1.0, 0.5]]


def test_windows():
    dec = wrapper()
    dec.set_window(None, first=1)
    assert called(dec, "mp3d_batch_set_window")[1:] == (1, 3, None, None)
    lo = np.array([0, 10], np.int64)
    dec.set_window(lo)
    assert called(dec, "mp3d_batch_set_window")[1:] == (0, 2, lo.ctypes.data, None)
    dec._L.peek["mp3d_batch_set_window"] = [(3, np.int64, 2), (4, np.int64, 2)]
    dec.set_window([0, 10], [5, None], first=2)
    assert called(dec, "mp3d_batch_set_window")[1:3] == (2, 2)
    assert [p.tolist() for p in dec._L.peeked] == [[0, 10], [5, M.WINDOW_NO_END]]
    for kw in ({}, {"first": 1}, {"first": 1, "n": 2}):
        lo, hi, fed = dec.sink_window(**kw)
        n = kw.get("n", 4 - kw.get("first", 0))
        assert called(dec, "mp3d_batch_sink_window")[1:] == (kw.get("first", 0), n) + tuple(
            host(x, (n,), np.int64) for x in (lo, hi, fed))


def test_housekeeping():
    dec = wrapper()
    dec.reset(), dec.sync(), dec.set_options(np.int64(1)), dec.set_timing(), dec.set_timing(False)
    a = called(dec, "mp3d_batch_reset", "mp3d_batch_sync", "mp3d_batch_set_options", "mp3d_batch_set_timing",
               "mp3d_batch_set_timing")
    assert [x[1:] for x in a] == [(), (), (M.OPT_CRC_CHECK,), (1,), (0,)] and type(a[2][1]) is int
    assert dec.kernel_times_us() == {"demux": 0.0, "huffman": 0.0, "synth": 0.0}
    called(dec, "mp3d_batch_kernel_times")
    for stage in ("resample", "feature", "loudness", "true_peak", "stretch", "limiter", "eq", "segment"):
        us = getattr(dec, stage + "_time_us")()
        assert us == 0.0 and type(us) is float
        called(dec, "mp3d_batch_%s_time" % stage)
    infos = dec.stream_info(np.int64(2))
    assert called(dec, "mp3d_batch_stream_info")[1] == 2
    assert len(infos) == 2 and all(isinstance(x, M.StreamInfo) for x in infos)
    h, L = dec._h, dec._L
    dec.close()
    dec.close()
    assert dec._h is None and L.calls == [("mp3d_batch_destroy", (h,))]


def test_state_blobs():
    dec, sb = wrapper(), M.state_bytes()
    blob = dec.get_state()
    assert called(dec, "mp3d_batch_get_state")[1:] == (0, 4, host(blob, (4, sb), np.uint8))
    blob = dec.get_state(first=1, n=2)
    assert called(dec, "mp3d_batch_get_state")[1:] == (1, 2, host(blob, (2, sb), np.uint8))
    dec.set_state(blob, first=2)
    assert called(dec, "mp3d_batch_set_state")[1:] == (2, 2, blob.ctypes.data)
    for bad in (lambda: dec.get_state(first=3, n=2), lambda: dec.set_state(blob, first=3),
                lambda: dec.set_state(blob.reshape(-1)[:-1]), lambda: dec.get_state(out=np.zeros(5, np.uint8))):
        with pytest.raises(ValueError):
            bad()
    assert not dec._L.calls


def test_long_streams():
    dec, data = wrapper(), np.zeros(64, np.uint8)
    for f32 in (False, True):
        pcm, infos, si = dec.decode_long(data, segment_frames=4, max_frames=3, f32=f32)
        a = called(dec, "mp3d_batch_decode_long")
        assert a[1:4] == (data.ctypes.data, 64, 4) and a[5:7] == (int(f32), 3)
        assert a[4] == host(pcm.base, (3, 2304), np.float32 if f32 else np.int16) and pcm.shape == (0, 2304)
        assert a[7] == host(infos.base, (3,), M.FRAME_INFO_DT) and isinstance(si, M.StreamInfo)
    pcm = dec.decode_long(data, pcm=np.zeros((5, 2304), np.int16))[0]
    assert called(dec, "mp3d_batch_decode_long")[6] == 5  # (max_frames: the rows of what is given)
    with pytest.raises(ValueError):
        dec.decode_long(data, max_frames=6, pcm=pcm.base)
    for f32, gapless in FLAGS:
        out = np.zeros((10, 2), np.float32 if f32 else np.int16)
        got, si, in_hz = dec.decode_long_packed(data, 44100, 2, 4, out=out, f32=f32, gapless=gapless)
        a = called(dec, "mp3d_batch_decode_long_packed")
        assert a[1:9] == (data.ctypes.data, 64, 4, 44100, 2, out.ctypes.data, int(f32), 10)
        assert a[10] == (M.LONG_GAPLESS if gapless else 0)
        assert got.base is out and got.shape == (0, 2) and in_hz == 0 and isinstance(si, M.StreamInfo)
    got = dec.decode_long_packed(data, 44100, 2, f32=False)[0]
    a = called(dec, "mp3d_batch_decode_long_packed")
    cap = M.long_packed_bound(data.tobytes(), 44100)
    assert a[8] == cap and a[3] == 32 and (a[6] is None or a[6] == host(got.base, (cap, 2), np.int16))


def test_chains_refuse_before_any_call():
    """decode_normalized and long_segments read the sinks' state first"""
    dec = wrapper()
    with pytest.raises(M.MP3DError, match="set_loudness and set_true_peak"):
        dec.decode_normalized(FRAMES, OFF, SZ, F)
    with pytest.raises(M.MP3DError, match="needs set_segments"):
        dec.long_segments(FRAMES)
    dec.set_output(HZ, CH), dec.set_loudness()
    with pytest.raises(M.MP3DError, match="set_loudness and set_true_peak"):
        dec.decode_normalized(FRAMES, OFF, SZ, F)
    dec.set_true_peak()
    with pytest.raises(M.MP3DError, match="needs set_limiter"):
        dec.decode_normalized(FRAMES, OFF, SZ, F, limit=True)
    dec.set_limiter(True, -2.0)
    with pytest.raises(M.MP3DError, match="not the limiter's ceiling"):
        dec.decode_normalized(FRAMES, OFF, SZ, F, limit=True)
    dec.set_limiter(False)
    with pytest.raises(M.MP3DError, match="needs set_limiter"):
        dec.decode_normalized(FRAMES, OFF, SZ, F, limit=True, max_dbtp=-2.0)
    assert {c[0] for c in dec._L.calls} <= {"mp3d_batch_set_output", "mp3d_batch_set_loudness",
                                            "mp3d_batch_set_true_peak", "mp3d_batch_set_limiter"}
