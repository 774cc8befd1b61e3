"""The packed sink's resampling filter (mp3d_resample_filter, host code, no
GPU) against an independent float64 restatement of the documented design
(include/mp3d.h "packed uniform-rate PCM sink"), the design's own frequency
response, and mp3d_packed_max_samples against the emit rule."""
import math

import numpy as np
import pytest

import mp3_amd

RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
PAIRS = [(a, b) for a in RATES for b in RATES if a != b]
# the pairs the design was checked for
NINE = [(44100, 48000), (44100, 16000), (48000, 8000), (8000, 48000), (22050, 44100), (11025, 32000), (44100, 8000),
        (32000, 48000), (48000, 44100)]


def sizes(in_hz, out_hz):
    g = math.gcd(in_hz, out_hz)
    L, M = out_hz // g, in_hz // g
    r = min(1.0, L / M)
    W = 24.0 / r
    # ceil(24 M / L) in integers: W is an exact integer whenever the float could be off
    T = 2 * (-(-24 * M // L) if L < M else 24)
    return L, M, r, W, T


def prototype(in_hz, out_hz):
    """h[p, j] of the formula in float64, before the per-phase normalisation."""
    L, M, r, W, T = sizes(in_hz, out_hz)
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(T, dtype=np.float64)[None, :]
    t = p / L - (j - (T // 2 - 1))
    inside = np.abs(t) < W
    w = np.where(inside, np.i0(9.0 * np.sqrt(np.where(inside, 1.0 - (t / W) ** 2, 0.0))) / np.i0(9.0), 0.0)
    return L, M, T, 0.88 * r * np.sinc(0.88 * r * t) * w


def restated(in_hz, out_hz):
    L, M, T, h = prototype(in_hz, out_hz)
    return L, M, T, h / h.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("in_hz,out_hz", PAIRS)
def test_taps_match_restatement(in_hz, out_hz):
    L, M, taps = mp3_amd.resample_filter(in_hz, out_hz)
    rl, rm, rt, ref = restated(in_hz, out_hz)
    assert (L, M, taps.shape) == (rl, rm, (rl, rt))
    assert taps.dtype == np.float32
    err = np.abs(taps.astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max()
    assert err <= 2.0 ** -24 * np.abs(ref).max(), (err, np.abs(ref).max())
    assert np.abs(taps.astype(np.float64).sum(axis=1) - 1.0).max() <= rt * 2.0 ** -24


def test_expected_tap_counts():
    assert all(sizes(a, b)[4] == 48 for a, b in PAIRS if b > a)
    assert sizes(44100, 16000)[4] == 134 and sizes(48000, 8000)[4] == 288
    assert max(sizes(a, b)[4] for a, b in PAIRS) == 288
    L, M, taps = mp3_amd.resample_filter(11025, 32000)
    assert taps.nbytes == 1280 * 48 * 4  # the largest table: more than the LDS holds


@pytest.mark.parametrize("hz", RATES)
def test_bypass(hz):
    L, M, taps = mp3_amd.resample_filter(hz, hz)
    assert (L, M) == (1, 1) and taps.shape == (1, 1) and taps[0, 0] == 1.0


def test_bad_rates():
    lib = mp3_amd.lib()
    assert lib.mp3d_resample_filter(44100, 44000, None, None, None, None, 0) == -1
    assert lib.mp3d_resample_filter(0, 48000, None, None, None, None, 0) == -1
    small = np.zeros(8, np.float32)  # a buffer too small for the taps is refused, not overrun
    assert lib.mp3d_resample_filter(44100, 48000, None, None, None, small.ctypes.data, small.size) == -1
    assert not small.any()
    assert lib.mp3d_packed_max_samples(44000, 1, 8000) == -1


@pytest.mark.parametrize("in_hz,out_hz", NINE)
def test_design_frequency_response(in_hz, out_hz):
    """The formula itself (not the code under test): the prototype low-pass,
    sampled at L * in_hz, is flat within 0.1 dB up to 0.79 of the lower
    Nyquist frequency and at -90 dB or lower from that frequency up."""
    L, M, T, h = prototype(in_hz, out_hz)
    # tap (p, j) sits at time t = p / L - (j - pre) input samples: index t * L + const
    pre = T // 2 - 1
    proto = np.zeros(L * T)
    p = np.arange(L)[:, None]
    j = np.arange(T)[None, :]
    proto[(p - (j - pre) * L + (T - 1 - pre) * L).ravel()] = h.ravel()
    n = 1 << 21
    assert proto.size < n
    H = np.abs(np.fft.rfft(proto, n))
    H /= H[0]
    f = np.arange(H.size) * (L * in_hz / n)
    nyq = min(in_hz, out_hz) / 2.0
    db = 20.0 * np.log10(np.maximum(H, 1e-12))
    passband = db[f <= 0.79 * nyq]
    stop = db[f >= nyq]
    print("passband %.4f .. %.4f dB, stopband max %.2f dB" % (passband.min(), passband.max(), stop.max()))
    assert passband.min() >= -0.1 and passband.max() <= 0.1
    assert stop.max() <= -90.0


def emitted(n, L, M, T):
    """Outputs emitted once n inputs were seen: those with n0 + T/2 <= n - 1."""
    post = T // 2 if T > 1 else 0
    m = 0
    while (m * M) // L + post <= n - 1:
        m += 1
    return m


@pytest.mark.parametrize("out_hz", RATES)
def test_packed_max_samples_is_the_emit_rule(out_hz):
    """The bound is the most one call can emit: a flushed call of `frames`
    frames that follows calls which left the longest pending tail (T/2 inputs
    seen, nothing emitted yet): ceil((N + T/2) L / M), the exact count of the
    emit rule plus the pending tail."""
    for frames in (1, 7, 32):
        per_rate = {}
        for in_hz in RATES:
            L, M, r, W, T = sizes(in_hz, out_hz) if in_hz != out_hz else (1, 1, 1.0, 0.0, 1)
            post = T // 2 if T > 1 else 0
            N = frames * (1152 if in_hz >= 32000 else 576)
            assert emitted(post, L, M, T) == 0  # the tail: seen, nothing emitted
            worst = -(-(N + post) * L // M)  # flushed lifetime total of N + post inputs
            # no earlier position leaves more for this call
            for seen in (0, 1, post - 1, post, post + 1, post + M, post + 7 * M + 3):
                if seen >= 0:
                    assert -(-(seen + N) * L // M) - emitted(seen, L, M, T) <= worst
            # an unflushed call emits exactly the emit rule's count
            assert emitted(N, L, M, T) == (max(0, -(-(N - post) * L // M)))
            per_rate[in_hz] = worst
        for min_hz in (8000, 16000, 32000, 44100, 48000):
            want = max(v for k, v in per_rate.items() if k >= min_hz)
            assert mp3_amd.packed_max_samples(out_hz, frames, min_hz) == want
        assert mp3_amd.packed_max_samples(out_hz, frames, 48001) == 0
