"""GPU: BatchDecoder.decode_long_packed (mp3d_batch_decode_long_packed): one
long stream, frame-parallel, straight to gapless interleaved PCM at one rate
and channel count.

The expected signal is always built from the plain float32 rows of
decode_long on a fresh handle (pinned to FFmpeg and the oracle by the rest of
the suite): untrimmed results must equal the packed sink's flushed output of
the same bytes bit for bit; trimmed ones are compared with the float64
reference of tests/test_gpu_packed.py on the trimmed, channel-mapped input,
within that file's bound (T + 2) * 2^-24 * S * A, and must not depend on the
segment length or the handle's width.
"""
import ctypes

import numpy as np
import pytest
import torch

import _gen
import _golden
import mp3_amd
import test_gpu_packed as PK
from mp3_amd import _build
from test_long_packed import audio_stream, tagged

pytestmark = pytest.mark.gpu

PATTERN = {True: np.float32(-777.25), False: np.int16(-1234)}
GEOM = (4, 3)  # (segment_frames, max_streams): a 16-frame stream takes two chunks
GEOMS = [(1, 1), (4, 3), (32, 64)]
MARGIN = 64  # samples of pattern kept past the bound


def golden(name):
    return _golden.case(name)[0]


def gen40():
    return _gen.stream(_gen.C3, 7, 40)[0]


def trim_stream(which):
    if which == "a":
        return golden("keypress_128k_js")
    if which == "b":
        return tagged(gen40(), 40, 576, 1500)
    if which == "c":
        s = audio_stream("lsf_22k_js")
        return tagged(s, len(mp3_amd.long_plan(s)[0]), 1700, 2000)
    if which == "d":
        return tagged(gen40(), 60, 576, 1500)
    if which == "e":
        return tagged(gen40(), 40, 576, 1500, with_count=False)
    if which == "f":
        return tagged(_gen.stream(_gen.C3, 7, 1)[0], 1, 2000, 0)
    raise KeyError(which)


_plain = {}


def plain(key, data):
    """(rows float32 [n, 2304], infos, StreamInfo) of decode_long on a fresh
    handle; computed once per stream."""
    if key not in _plain:
        _plain[key] = mp3_amd.BatchDecoder(64, 32 + 11).decode_long(data, 32, f32=True)
    return _plain[key]


def raw_call(dec, data, L, hz, ch, out, f32, cap, gapless):
    """The C call: (rc, out_samples, in_hz, StreamInfo)."""
    nbytes = data.numel() if hasattr(data, "numel") else len(data)
    dp, k1 = mp3_amd._ptr(data)
    op, k2 = mp3_amd._ptr(out)
    n, in_hz, si = ctypes.c_longlong(-7), ctypes.c_int(-7), mp3_amd.StreamInfo()
    rc = dec._L.mp3d_batch_decode_long_packed(dec._h, dp, nbytes, L, hz, ch, op, int(f32), cap, ctypes.byref(n),
                                              mp3_amd.LONG_GAPLESS if gapless else 0, ctypes.byref(si),
                                              ctypes.byref(in_hz))
    return rc, n.value, in_hz.value, si


def long_run(data, fmt, f32=True, gapless=True, geom=GEOM):
    """(samples [n, ch], in_hz, StreamInfo) on a fresh handle, after checking
    that the bytes of out past the count still hold the pattern."""
    L, streams = geom
    dec = mp3_amd.BatchDecoder(streams, L + 11)
    cap = mp3_amd.long_packed_bound(data, fmt[0]) + MARGIN
    out = np.full((cap, fmt[1]), PATTERN[f32], np.float32 if f32 else np.int16)
    got, si, in_hz = dec.decode_long_packed(data, fmt[0], fmt[1], segment_frames=L, out=out, f32=f32, gapless=gapless)
    assert got.base is out or got is out
    assert len(got) <= cap - MARGIN  # long_packed_bound is a bound
    assert (out[len(got):] == PATTERN[f32]).all()
    return got.copy(), in_hz, si


def packed_run(data, fmt, f32=True):
    """The same bytes as ONE stream through the batched packed sink, flushed."""
    n = max(1, len(mp3_amd.long_plan(data)[0]))
    dec = mp3_amd.BatchDecoder(1, n)
    dec.set_output(*fmt)
    blob = np.frombuffer(data + b"\0" * 64, np.uint8)
    out, counts, _ = dec.decode_packed(blob, [0], [len(data)], n, f32=f32, flush=True)
    assert counts[0] >= 0
    return out[0, : counts[0]].copy()


def same_bits(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = np.uint32 if a.dtype == np.float32 else np.uint16
    assert np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u)), what


# ---- 1. bit-identical to the packed sink, untrimmed -------------------------
UNTRIMMED = [(nm, fmt) for nm in ["c3_s0", "c5_dual_32k_vbr", "c5_mono_48k_crc", "lsf_22k_js", "lsf_8k_js",
                                  "edge_bv_drop", "edge_garbage", "long_c3_512"]
             for fmt in [(48000, 2), (16000, 1), (44100, 2)]] + [("lsf_11k_ms_is", (32000, 2))]


def check_untrimmed(data, fmt, geom=GEOM):
    outs = []
    for f32 in (True, False):
        got, in_hz, _ = long_run(data, fmt, f32=f32, gapless=False, geom=geom)
        want = packed_run(data, fmt, f32=f32)
        print("%s f32=%d: %d samples from %d Hz" % (fmt, f32, len(got), in_hz))
        same_bits(got, want, (fmt, f32))
        outs.append(got)
    return outs


@pytest.mark.parametrize("name,fmt", UNTRIMMED)
def test_untrimmed_equals_the_packed_sink(name, fmt):
    data = golden(name)
    f, q = check_untrimmed(data, fmt)
    assert len(f) > 0
    rows, infos, _ = plain(name, data)
    hz, x = PK.mapped_input(rows, infos, fmt[1])
    L, M = PK.filt(hz, fmt[0])[:2]
    assert len(f) == -(-x.shape[0] * L // M)


# ---- 2. chunk and segment invariance ----------------------------------------
def invariant(data, fmt, gapless, f32=True):
    runs = [long_run(data, fmt, f32=f32, gapless=gapless, geom=g) for g in GEOMS]
    for g, r in zip(GEOMS[1:], runs[1:]):
        same_bits(r[0], runs[0][0], (fmt, g))
        assert r[1] == runs[0][1]
    return runs[0][0]


@pytest.mark.parametrize("name,fmt", [("long_c3_512", (48000, 2)), ("long_c3_512", (16000, 1)),
                                      ("lsf_8k_js", (48000, 2)), ("lsf_8k_js", (16000, 1)),
                                      ("c5_mono_48k_crc", (8000, 1)), ("edge_garbage", (48000, 2))])
def test_geometry_invariance(name, fmt):
    """(1, 1): every chunk is one frame, so every filter span straddles
    chunks (48 kHz -> 8 kHz: 288 taps over 1152-sample chunks)."""
    assert len(invariant(golden(name), fmt, gapless=False)) > 0


def test_geometry_invariance_with_empty_chunks(name="edge_bv_drop"):
    """With (1, 1) a slot without audio (a dropped frame) is a whole chunk
    without input."""
    data = golden(name)
    _, infos, _ = plain(name, data)
    assert (infos["samples"] == 0).any()
    for fmt in [(48000, 2), (16000, 1)]:
        assert len(invariant(data, fmt, gapless=False)) > 0


@pytest.mark.parametrize("fmt", [(48000, 2), (16000, 1)])
def test_geometry_invariance_of_the_trim(fmt):
    """Stream (b): with (1, 1) the first chunk with input keeps 47 samples
    after the head trim, fewer than T - 1 at 44.1 -> 16 kHz (133)."""
    assert len(invariant(trim_stream("b"), fmt, gapless=True)) > 0


# ---- 3. trim, values --------------------------------------------------------
@pytest.mark.parametrize("which", list("abcdef"))
@pytest.mark.parametrize("fmt", [(48000, 2), (16000, 1)])
def test_trim_values(which, fmt):
    data = trim_stream(which)
    rows, infos, si = plain("trim_" + which, data)
    assert si.has_lame == 1
    planar = mp3_amd.pcm_to_planar(rows, infos)
    n_trim = mp3_amd.gapless_trim(planar, si).shape[1]
    hz, x = PK.mapped_input(rows, infos, fmt[1])
    xt = np.ascontiguousarray(mp3_amd.gapless_trim(x.T, si).T)
    assert xt.shape[0] == n_trim
    if which == "d":
        assert si.end_sample > planar.shape[1]  # past the data: stop = N
    if which == "e":
        assert si.end_sample == -1 and n_trim == planar.shape[1] - si.skip_samples
    if which == "f":
        assert n_trim == 0
    y, bound = PK.reference(xt, hz, fmt[0])
    L, M = PK.filt(hz, fmt[0])[:2]
    got, in_hz, got_si = long_run(data, fmt, gapless=True)
    assert in_hz == hz and bytes(got_si) == bytes(si)
    assert len(got) == -(-n_trim * L // M) == y.shape[0], (len(got), n_trim, y.shape)
    err = float(np.abs(got.astype(np.float64) - y).max()) if y.size else 0.0
    print("%s %s: N' %d, %d samples, max err %.3g, bound %.3g" % (which, fmt, n_trim, len(got), err, bound))
    assert err <= bound


@pytest.mark.parametrize("fmt", [(48000, 2), (16000, 1)])
def test_without_the_flag_nothing_is_trimmed(fmt):
    check_untrimmed(trim_stream("b"), fmt)


# ---- 4. trim, exact ---------------------------------------------------------
@pytest.mark.parametrize("which,fmt", [("a", (44100, 2)), ("b", (44100, 2)), ("c", (22050, 2))])
def test_trim_bypass_is_exact(which, fmt):
    data = trim_stream(which)
    rows, infos, si = plain("trim_" + which, data)
    want = np.ascontiguousarray(mp3_amd.gapless_trim(mp3_amd.pcm_to_planar(rows, infos), si).T)
    assert want.shape[1] == fmt[1] and want.shape[0] > 0
    got, in_hz, _ = long_run(data, fmt, gapless=True)
    assert in_hz == fmt[0]
    same_bits(got, want, which)


def test_trim_bypass_int16_matches_ffmpeg():
    ref = np.load(_golden.GOLDEN / "keypress_128k_js.tagged.pcm16.npy")
    got, _, _ = long_run(trim_stream("a"), (44100, 2), f32=False, gapless=True)
    assert got.T.shape == ref.shape, (got.T.shape, ref.shape)
    assert int(np.abs(got.T.astype(np.int32) - ref.astype(np.int32)).max()) <= 1


# ---- 5. device buffers and capacity -----------------------------------------
@pytest.mark.parametrize("fmt", [(48000, 2), (16000, 1)])
@pytest.mark.parametrize("f32", [True, False])
def test_device_buffers(fmt, f32):
    data = trim_stream("b")
    want, want_hz, _ = long_run(data, fmt, f32=f32)
    L, streams = GEOM
    dec = mp3_amd.BatchDecoder(streams, L + 11)
    cap = mp3_amd.long_packed_bound(data, fmt[0]) + MARGIN
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out = torch.full((cap, fmt[1]), float(PATTERN[f32]), dtype=torch.float32 if f32 else torch.int16, device="cuda")
    got, _, in_hz = dec.decode_long_packed(d_in, fmt[0], fmt[1], segment_frames=L, out=out, f32=f32)
    assert in_hz == want_hz
    same_bits(got.cpu().numpy(), want)
    assert (out[len(got):].cpu().numpy() == PATTERN[f32]).all()


@pytest.mark.parametrize("device", [False, True])
def test_capacity(device):
    data, fmt = trim_stream("b"), (48000, 2)
    full, _, _ = long_run(data, fmt)
    cap = len(full) - 1000
    L, streams = GEOM
    dec = mp3_amd.BatchDecoder(streams, L + 11)
    out = np.full((cap + MARGIN, 2), PATTERN[True], np.float32)
    if device:
        out = torch.from_numpy(out).cuda()
    rc, n, in_hz, _ = raw_call(dec, data, L, 48000, 2, out, True, cap, True)
    assert rc == -5 and n == len(full) and in_hz == 44100
    host = out.cpu().numpy() if device else out
    same_bits(host[:cap], full[:cap])
    assert (host[cap:] == PATTERN[True]).all()


def test_argument_errors():
    data = trim_stream("b")
    L, streams = GEOM
    dec = mp3_amd.BatchDecoder(streams, L + 11)
    flat = torch.zeros(2 * (mp3_amd.long_packed_bound(data, 48000) + 1) + 1, dtype=torch.float32, device="cuda")
    out = flat[1:]  # 4 bytes off an 8-byte sample frame
    assert raw_call(dec, data, L, 48000, 2, out, True, out.numel() // 2, True)[0] == -1
    assert not flat.any().item()
    host = np.zeros((mp3_amd.long_packed_bound(data, 48000), 2), np.float32)
    for hz, ch, seg in [(44000, 2, L), (48000, 3, L), (48000, 2, 0)]:
        assert raw_call(dec, data, seg, hz, ch, host, True, len(host), True)[0] == -1
    assert not host.any()
    dp, keep = mp3_amd._ptr(data)
    assert dec._L.mp3d_batch_decode_long_packed(dec._h, dp, len(data), L, 48000, 2, host.ctypes.data, 1, len(host), None,
                                                0, None, None) == -1
    # a handle too short for the segments' warm-up: as decode_long
    long_data = golden("long_c3_512")
    small = mp3_amd.BatchDecoder(4, 32 + 3)
    with pytest.raises(mp3_amd.MP3DError, match="-5"):
        small.decode_long(long_data, 32)
    with pytest.raises(mp3_amd.MP3DError, match="-5"):
        small.decode_long_packed(long_data, 48000, 2, segment_frames=32)


# ---- 6. the handle is left alone --------------------------------------------
@pytest.fixture(scope="module")
def batch():
    return PK.Batch()


@pytest.mark.parametrize("long_fmt", [(48000, 2), (16000, 1)])
def test_the_handle_is_left_alone(batch, long_fmt):
    """A long call between two packed calls, to another format than the
    handle's and to the same (then it borrows the handle's filter table)."""
    offs5, sizes5 = batch.geom(0, 5)
    offs11, sizes11 = batch.geom(5, 16)
    data = golden("c3_s0")

    def packed(with_long):
        dec = mp3_amd.BatchDecoder(batch.n, 16)
        dec.set_output(16000, 1)
        first = dec.decode_packed(batch.blob, offs5, sizes5, 5)
        if with_long:
            got, _, _ = dec.decode_long_packed(data, long_fmt[0], long_fmt[1], segment_frames=4, gapless=False)
            same_bits(got, long_run(data, long_fmt, gapless=False)[0])
        return first, dec.decode_packed(batch.blob, offs11, sizes11, 11, flush=True)

    def plain_calls(with_long):
        dec = mp3_amd.BatchDecoder(batch.n, 16)
        dec.set_options(mp3_amd.OPT_CRC_CHECK)
        first = dec.decode(batch.blob, offs5, sizes5, 5, f32=True)
        if with_long:
            dec.decode_long_packed(data, long_fmt[0], long_fmt[1], segment_frames=4)
        return first, dec.decode(batch.blob, offs11, sizes11, 11, f32=True), dec.get_state(0, batch.n)

    for run in (packed, plain_calls):
        want, got = run(False), run(True)
        for w, g in zip(want, got):
            for x, y in zip(w, g) if isinstance(w, tuple) else [(w, g)]:
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), run.__name__
    assert want[1][0].any()


# ---- 7. poison ---------------------------------------------------------------
def poison_cases():
    """Test 1 on c3_s0 and test 3 (b), every format: the samples."""
    out = []
    for fmt in [(48000, 2), (16000, 1), (44100, 2)]:
        out += check_untrimmed(golden("c3_s0"), fmt)
    for fmt in [(48000, 2), (16000, 1)]:
        out.append(long_run(trim_stream("b"), fmt, gapless=True)[0])
    return out


def test_poison(monkeypatch):
    want = poison_cases()
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    got = poison_cases()
    for w, g in zip(want, got):
        same_bits(g, w)


def test_workgroup_lds_poison_build():
    want = poison_cases()
    with mp3_amd.library(_build.WGLDS_LIB):
        got = poison_cases()
    for w, g in zip(want, got):
        same_bits(g, w)
