"""No GPU: the pitch sink's definition (include/mp3d.h "pitch sink") restated
in numpy with int64, its host-only exports, its bounds and what the wrapper
hands to the library.

pitch_ref and pitch_by_call are the reference of tests/test_gpu_pitch.py.  They
assert the integer bounds the header states (|r| <= 1024, |X| < 2^30,
D < 2^32) on every frame they see.
"""
import ctypes

import numpy as np
import pytest

import mp3_amd as M
import test_wrapper_calls as tw

DT = M.PITCH_FRAME_DT
DEFAULT = (60, 500, 154)


# ---- the definition ---------------------------------------------------------------
def hop(fs):
    return (fs + 50) // 100


def lags(fs, fmin, fmax):
    """(tmin, tmax, SPAN)"""
    tmin, tmax = -(-fs // fmax), fs // fmin
    return tmin, tmax, 2 * hop(fs) + tmax + 1


def quantise(x):
    """float32 [n] or [n, ch] -> q int64 [n]: the tempo sink's mono mix, the packed sink's int16"""
    x = np.asarray(x, np.float32)
    m = x if x.ndim == 1 else x[:, 0] if x.shape[1] == 1 else np.float32(0.5) * (x[:, 0] + x[:, 1])
    v = m.astype(np.float64) * 32768.0  # (exact)
    return np.clip(np.floor(v + 0.5), -32768, 32767).astype(np.int64)


def known(N, H, SPAN):
    return 0 if N < SPAN else (N - SPAN) // H + 1


def frame_record(xf, fs, W, tmin, tmax, theta):
    """one frame's record from its SPAN samples (int64)"""
    T = tmax + 1
    mx = int(np.abs(xf).max())
    sh = max(0, mx.bit_length() - 10)
    r = xf >> sh
    assert np.abs(r).max() <= 1024
    win = np.lib.stride_tricks.sliding_window_view(r, W)  # win[tau] = r[tau .. tau + W)
    X = win[1: T + 1] @ r[:W]
    assert np.abs(X).max() < 2 ** 30
    Q = np.concatenate([[0], np.cumsum(r * r)])
    tau = np.arange(1, T + 1)
    D = np.concatenate([[0], Q[W] + (Q[tau + W] - Q[tau]) - 2 * X])  # D[tau], D[0] = 0
    assert D.min() >= 0 and D.max() < 2 ** 32
    assert np.array_equal(D[1:], ((r[:W][None, :] - win[1: T + 1]) ** 2).sum(axis=1))
    S = np.cumsum(D)
    cand = np.arange(tmin, tmax + 1)
    lhs, rhs = D[cand] * cand * 1024, theta * S[cand]
    assert max(lhs.max(initial=0), rhs.max(initial=0)) < 2 ** 53
    ok = np.nonzero(lhs < rhs)[0]
    if not len(ok):
        return (0.0, 0.0, 0, sh)
    t = int(cand[ok[0]])
    while t < tmax and D[t + 1] < D[t]:
        t += 1
    a, b, c = int(D[t - 1]), int(D[t]), int(D[t + 1])
    den = a - 2 * b + c
    delta = 0.5 * float(a - c) / float(den) if den > 0 else 0.0
    delta = min(max(delta, -1.0), 1.0)
    f0 = np.float32(float(fs) / (float(t) + delta))
    per = np.float32(max(0.0, 1.0 - float(b * t) / float(int(S[t]))))
    return (f0, per, t, sh)


def pitch_ref(q, fs, fmin, fmax, theta, flush):
    """the records of a stream of quantised samples q fed to a fresh slot in one call"""
    q = np.asarray(q, np.int64)
    H = hop(fs)
    tmin, tmax, SPAN = lags(fs, fmin, fmax)
    N = len(q)
    nf = -(-N // H) if flush else known(N, H, SPAN)
    qz = np.concatenate([q, np.zeros(SPAN + H, np.int64)])
    out = np.zeros(nf, DT)
    for f in range(nf):
        out[f] = frame_record(qz[f * H: f * H + SPAN], fs, 2 * H, tmin, tmax, theta)
    return out


def pitch_by_call(q, fs, fmin, fmax, theta, cuts, flush_last):
    """[records of call i] when the stream is fed in calls that end at cuts[i]; the last one flushes if asked"""
    H = hop(fs)
    SPAN = lags(fs, fmin, fmax)[2]
    full = pitch_ref(q[: cuts[-1]], fs, fmin, fmax, theta, True)
    out, have = [], 0
    for i, c in enumerate(cuts):
        k = len(full) if flush_last and i == len(cuts) - 1 else known(c, H, SPAN)
        # (a frame known without a flush reads no sample past the call's end: its record is the flushed stream's)
        out.append(full[have:k])
        have = k
    return out


def same(a, b):
    return a.dtype == b.dtype == DT and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- signals ----------------------------------------------------------------------
def harmonic(fs, f, n, amp=0.5, missing=False, noise=0.02, seed=0):
    """a harmonic complex of f Hz (six partials, 1/k, the first left out when `missing`), with white noise"""
    t = np.arange(n) / fs
    ks = [k for k in range(2 if missing else 1, 8) if k * f < 0.45 * fs][:6]
    x = sum(np.sin(2 * np.pi * k * f * t + 0.3 * k) / k for k in ks)
    x = x / np.abs(x).max()
    x = x + noise * np.random.default_rng(seed).standard_normal(n)
    return (amp * x / np.abs(x).max()).astype(np.float32)


def square(period, n, amp):
    return np.where(np.arange(n) % period < period // 2, amp, -amp).astype(np.int64)


WORST = {  # int16 signals at the edges of the integer bounds
    "alt_full": lambda n: np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int64),
    "alt_2047": lambda n: np.where(np.arange(n) % 2 == 0, 2047, -2047).astype(np.int64),
    "square_96": lambda n: square(96, n, 32767),
    "dc_min": lambda n: np.full(n, -32768, np.int64),
}


# ---- the definition's bounds and properties -----------------------------------------
@pytest.mark.parametrize("name", sorted(WORST))
def test_worst_cases_hold_the_integer_bounds(name):
    fs = 48000
    q = WORST[name](3 * hop(fs) + lags(fs, 50, 2000)[2])
    rec = pitch_ref(q, fs, 50, 2000, 154, True)  # (the bounds are asserted inside)
    assert len(rec) == -(-len(q) // hop(fs))
    if name == "dc_min":
        assert (rec["lag"][:3] == 0).all() and (rec["shift"][:3] == 6).all()  # S = 0: unvoiced
    if name == "square_96":
        assert (rec["lag"][:3] == 96).all() and (rec["periodicity"][:3] == 1).all()  # D(96) = D(192) = 0: the smaller


@pytest.mark.parametrize("fs", (8000, 16000, 44100, 48000))
@pytest.mark.parametrize("f", (70.0, 110.0, 233.3, 440.0))
def test_tones_come_back_within_one_lag(fs, f):
    n = lags(fs, *DEFAULT[:2])[2] + 2 * hop(fs)
    for missing in (False, True):
        lag = {}
        for amp in (0.5, 0.003):
            rec = pitch_ref(quantise(harmonic(fs, f, n, amp, missing)), fs, *DEFAULT, False)
            assert len(rec) == 3 and (rec["lag"] > 0).all(), (missing, amp)
            assert (np.abs(fs / rec["f0_hz"].astype(np.float64) - fs / f) <= 1).all(), (missing, amp, rec)
            assert (rec["periodicity"] > 0.8).all()
            lag[amp] = rec["lag"]
        assert (np.abs(lag[0.5] - lag[0.003]) <= 1).all()


def test_scale_moves_the_lag_by_at_most_one():
    fs = 16000
    x = harmonic(fs, 150.0, 2000, 1.0, noise=0.0)
    loud = pitch_ref(quantise(x), fs, *DEFAULT, False)
    quiet = pitch_ref(quantise(x * np.float32(10 ** (-44 / 20))), fs, *DEFAULT, False)
    assert len(loud) > 5 and (loud["lag"] > 0).all() and (np.abs(loud["lag"] - quiet["lag"]) <= 1).all()
    assert loud["shift"].min() >= 5 and quiet["shift"].max() == 0


@pytest.mark.parametrize("fs", (8000, 48000))
def test_noise_and_silence_are_unvoiced(fs):
    n = lags(fs, *DEFAULT[:2])[2] + 4 * hop(fs)
    noise = np.random.default_rng(fs).uniform(-0.5, 0.5, n).astype(np.float32)
    for q in (quantise(noise), np.zeros(n, np.int64)):
        rec = pitch_ref(q, fs, *DEFAULT, True)
        assert len(rec) == -(-n // hop(fs)) and not rec["lag"].any() and not rec["f0_hz"].any()
        assert not rec["periodicity"].any()


def test_an_empty_lag_range_is_unvoiced():
    fs = 11025
    assert M.pitch_span(fs, 1999, 2000)[1:] == (6, 5)
    rec = pitch_ref(quantise(harmonic(fs, 2000.0, 600)), fs, 1999, 2000, 1024, True)
    assert len(rec) and not rec["lag"].any()


def test_exact_ties_take_the_smaller_lag():
    fs = 48000
    q = square(96, 4000, 1000)
    rec = pitch_ref(q, fs, 50, 2000, 154, False)
    assert len(rec) and (rec["lag"] == 96).all() and (rec["f0_hz"] == 500.0).all()


def test_by_call_is_the_single_call_cut_up():
    fs = 8000
    q = quantise(harmonic(fs, 110.0, 1500))
    whole = pitch_ref(q, fs, *DEFAULT, True)
    parts = pitch_by_call(q, fs, *DEFAULT, [0, 1, 400, 401, 1200, 1500, 1500], True)
    assert same(np.concatenate(parts), whole) and len(parts[0]) == 0 and len(parts[-1]) > 0
    unflushed = pitch_by_call(q, fs, *DEFAULT, [700, 1500], False)
    assert same(np.concatenate(unflushed), pitch_ref(q, fs, *DEFAULT, False))


# ---- the host exports ---------------------------------------------------------------
def limits(fs):
    top = min(fs // 4, 2000)
    return [DEFAULT[:2], (50, top), (top - 1, top), (50, 51), (50, 400), (200, 300)]


@pytest.mark.parametrize("fs", M.RATES)
def test_pitch_span(fs):
    for fmin, fmax in limits(fs):
        tmin, tmax, span = lags(fs, fmin, fmax)
        assert M.pitch_span(fs, fmin, fmax) == (span, tmin, tmax)
        # (limits one hertz apart can leave no whole lag between them: 11 025 Hz, 1999 .. 2000 gives 6 > 5)
        assert 4 <= tmin and tmax <= 960 and span <= 1921 and (tmin <= tmax or fmax - fmin == 1)
    assert 4 * min(fs // 4, 2000) == fs or fs > 8000  # (4 fmax == fs exists at 8 kHz)
    L = M.lib()
    assert L.mp3d_pitch_span(fs, 60, 500, None, None) == lags(fs, 60, 500)[2]  # null pointers
    one = ctypes.c_int(-1)
    assert L.mp3d_pitch_span(fs, 60, 500, None, ctypes.byref(one)) > 0 and one.value == fs // 60
    top = min(fs // 4, 2000)
    for bad in [(49, 500), (60, 60), (61, 60), (60, top + 1), (60, 2001), (0, 500), (-5, 500)]:
        one.value = -1
        assert L.mp3d_pitch_span(fs, bad[0], bad[1], ctypes.byref(one), None) == -1, bad
        assert one.value == -1  # nothing written


def test_pitch_span_edges_and_bad_rates():
    assert M.pitch_span(48000, 50, 2000) == (1921, 24, 960)
    assert M.pitch_span(8000, 1999, 2000) == (2 * 80 + 5, 4, 4)
    for hz in (0, 44000, 96000, -8000):
        with pytest.raises(M.MP3DError):
            M.pitch_span(hz, 60, 500)
        with pytest.raises(M.MP3DError):
            M.pitch_max_frames(hz, 100, 60)


@pytest.mark.parametrize("fs", M.RATES)
def test_pitch_max_frames(fs):
    H = hop(fs)
    top = min(fs // 4, 2000)
    for fmin in (50, 60, top - 1):
        span = 2 * H + fs // fmin + 1
        for n in (0, 1, H - 1, H, 12345, 2 ** 31 - 1):
            assert M.pitch_max_frames(fs, n, fmin) == (n + span + H - 2) // H
    L = M.lib()
    for n, fmin in [(-1, 60), (2 ** 31, 60), (10, 49), (10, top), (10, 2000), (10, 0)]:
        assert L.mp3d_pitch_max_frames(fs, n, fmin) == -1, (n, fmin)


# ---- the frame bound and the carry ----------------------------------------------------
@pytest.mark.parametrize("H,SPAN", [(1, 3), (2, 5), (3, 11), (5, 12), (7, 15)])
def test_frame_bound_by_brute_force(H, SPAN):
    """every pending length and every count: a call never emits more than the bound, and reaches it"""
    slack = {}
    for N0 in range(0, 3 * SPAN + 3 * H):
        assert N0 - known(N0, H, SPAN) * H <= SPAN - 1  # what the carry holds
        for c in range(0, 4 * SPAN):
            bound = (c + SPAN + H - 2) // H
            plain = known(N0 + c, H, SPAN) - known(N0, H, SPAN)
            flushed = -(-(N0 + c) // H) - known(N0, H, SPAN)
            assert 0 <= plain <= flushed <= bound, (N0, c)
            slack[c] = min(slack.get(c, bound), bound - flushed)
    assert set(slack.values()) == {0}  # reached for every count


def test_the_carry_of_the_real_formats():
    for fs in M.RATES:
        H = hop(fs)
        SPAN = lags(fs, 50, min(fs // 4, 2000))[2]
        assert SPAN - 1 <= 1920
        assert max(N - known(N, H, SPAN) * H for N in range(0, 3 * SPAN)) == SPAN - 1


# ---- what the wrapper hands to the library ---------------------------------------------
ALONE = "h samples ss counts n out stride ocounts flags stream".split()
DECODE = "h frames off sz n F out stride ocounts flags infos stream".split()
FMIN = 70


def make(mode):
    dec = tw.wrapper()
    if mode == "fresh":
        return dec, 0, False
    dec.set_output(tw.HZ, tw.CH)
    if mode == "on":
        dec.set_pitch(True, fmin=FMIN, fmax=400)
    dec._L.calls.clear()
    return dec, tw.HZ, mode == "on"


def test_set_pitch():
    dec = tw.wrapper()
    dec.set_output(48000, 2)
    tw.called(dec, "mp3d_batch_set_output")
    assert dec._pitch is None
    dec.set_pitch()
    a = tw.called(dec, "mp3d_batch_set_pitch")
    assert a[1:] == (1, 60, 500, 154) and all(type(v) is int for v in a[1:]) and dec._pitch == 60
    dec.set_pitch(True, fmin=np.int64(50), fmax=2000.0, threshold=1.0)
    assert tw.called(dec, "mp3d_batch_set_pitch")[1:] == (1, 50, 2000, 1024) and dec._pitch == 50
    dec.set_pitch(False)
    assert tw.called(dec, "mp3d_batch_set_pitch")[1:] == (0, 60, 500, 154) and dec._pitch is None
    dec.set_pitch(True, threshold=0.001)
    assert tw.called(dec, "mp3d_batch_set_pitch")[4] == 1
    dec.set_output(48000, 2)  # a change of the format turns the sink off
    assert dec._pitch is None and "_pitch" in M.BatchDecoder._AFTER_PACKED
    us = dec.pitch_time_us()
    assert us == 0.0 and type(us) is float
    tw.called(dec, "mp3d_batch_set_output", "mp3d_batch_pitch_time")
    with pytest.raises(M.MP3DError, match="needs set_pitch"):
        dec.long_pitch(tw.FRAMES)
    assert not dec._L.calls


@pytest.mark.parametrize("mode", tw.MODES)
@pytest.mark.parametrize("ss", (0, 5))
@pytest.mark.parametrize("flush", (False, True))
def test_pitch_alone_defaults(mode, ss, flush):
    dec, hz, on = make(mode)
    smp = np.zeros((tw.N, ss, max(tw.CH, 1)), np.float32)
    out, oc = dec.pitch(smp, tw.COUNTS, flush=flush)
    a = dict(zip(ALONE, tw.called(dec, "mp3d_batch_pitch")))
    tw.stage_head(a, smp, ss)
    stride = M.pitch_max_frames(hz, ss, FMIN) if on else 1
    assert a["stride"] == stride and type(a["stride"]) is int
    assert a["out"] == tw.host(out, (tw.N, stride), DT) and a["ocounts"] == tw.host(oc, (tw.N,), np.int32)
    assert a["flags"] == (M.PACK_FLUSH if flush else 0) and a["stream"] is None


@pytest.mark.parametrize("mode", tw.MODES)
@pytest.mark.parametrize("flush,gapless", tw.FLAGS)
def test_decode_pitch_defaults(mode, flush, gapless):
    dec, hz, on = make(mode)
    out, oc, infos = dec.decode_pitch(tw.FRAMES, tw.OFF, tw.SZ, tw.F, flush=flush, gapless=gapless)
    a = dict(zip(DECODE, tw.called(dec, "mp3d_batch_decode_pitch")))
    tw.decode_head(a, infos)
    stride = M.pitch_max_frames(hz, M.packed_max_samples(hz, tw.F), FMIN) if on else 1
    assert a["stride"] == stride and type(a["stride"]) is int
    assert a["out"] == tw.host(out, (tw.N, stride), DT) and not out.view(np.uint8).any()
    assert a["ocounts"] == tw.host(oc, (tw.N,), np.int32) and not oc.any()
    assert a["flags"] == (M.PACK_FLUSH if flush else 0) | (M.PACK_GAPLESS if gapless else 0)
    assert a["stream"] is None


def test_given_buffers_and_strides():
    dec, hz, on = make("on")
    smp = np.zeros((tw.N, 5, tw.CH), np.float32)
    out, oc = np.zeros((tw.N, 7), DT), np.zeros(tw.N, np.int32)
    r = dec.pitch(smp, tw.COUNTS, out=out, out_counts=oc, stream=77)
    a = dict(zip(ALONE, tw.called(dec, "mp3d_batch_pitch")))
    assert r[0] is out and r[1] is oc and (a["out"], a["stride"], a["ocounts"]) == (out.ctypes.data, 7, oc.ctypes.data)
    assert tw.stream_of(a["stream"]) == 77
    infos = np.zeros((tw.N, tw.F), M.FRAME_INFO_DT)
    r = dec.decode_pitch(tw.FRAMES, tw.OFF, tw.SZ, tw.F, out=out, counts=oc, infos=infos, stream=77)
    a = dict(zip(DECODE, tw.called(dec, "mp3d_batch_decode_pitch")))
    assert r == (out, oc, infos) and (a["out"], a["stride"], a["ocounts"]) == (out.ctypes.data, 7, oc.ctypes.data)
    assert tw.stream_of(a["stream"]) == 77
    r = dec.decode_pitch(tw.FRAMES, tw.OFF, tw.SZ, tw.F, stride=np.int64(3))
    a = dict(zip(DECODE, tw.called(dec, "mp3d_batch_decode_pitch")))
    assert a["stride"] == 3 and type(a["stride"]) is int and a["out"] == tw.host(r[0], (tw.N, 3), DT)
    r = dec.pitch(smp, tw.COUNTS, stride=3)
    a = dict(zip(ALONE, tw.called(dec, "mp3d_batch_pitch")))
    assert a["stride"] == 3 and a["out"] == tw.host(r[0], (tw.N, 3), DT)
    with pytest.raises(ValueError):
        dec.decode_pitch(tw.FRAMES, [0, 8], [8], tw.F)
    assert not dec._L.calls


def test_the_record_dtype():
    assert DT.itemsize == 16 and DT.names == ("f0_hz", "periodicity", "lag", "shift")
    assert [DT.fields[k][1] for k in DT.names] == [0, 4, 8, 12]
