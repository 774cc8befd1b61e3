"""The host-only half of true peak and gain (include/mp3d.h "true peak and
gain"; no GPU needed): the oversampling filter against the header's formula in
float64 numpy, its structure, the three filter facts DESIGN.md section 4f
quotes, argument errors and the exports.

The restatement below (taps64, truepeak64, gain64, int16_of) is also the
reference of tests/test_gpu_normalize.py."""
import ctypes
import math

import numpy as np

import mp3_amd

NEW = ["mp3d_truepeak_filter", "mp3d_batch_set_true_peak", "mp3d_batch_true_peak", "mp3d_batch_decode_measure",
       "mp3d_batch_normalize_gain", "mp3d_batch_apply_gain", "mp3d_batch_true_peak_time"]
R, T, PRE, POST = 4, 12, 5, 6


# ---- the definition in float64 ---------------------------------------------------
def taps64():
    """The header's formula in float64, rounded to float32: [4, 12]."""
    taps = np.zeros((R, T), np.float64)
    taps[0, PRE] = 1.0
    j = np.arange(T, dtype=np.float64)
    for p in range(1, R):
        t = p / 4.0 - (j - PRE)
        w = np.where(np.abs(t) < 6.0, np.i0(6.0 * np.sqrt(np.maximum(1.0 - (t / 6.0) ** 2, 0.0))) / np.i0(6.0), 0.0)
        h = np.sinc(t) * w
        taps[p] = h / h.sum()
    return taps.astype(np.float32)


def oversample64(x):
    """u float64 [N, R, ch] of x float32 [N, ch]: every index of a flushed
    stream, float32 taps, float64 arithmetic."""
    x = np.asarray(x, np.float32)
    N, ch = x.shape
    taps = taps64().astype(np.float64)
    xp = np.zeros((N + T - 1, ch), np.float64)
    xp[PRE:PRE + N] = x
    u = np.zeros((N, R, ch), np.float64)
    for c in range(ch):
        for p in range(R):
            if N:
                u[:, p, c] = np.correlate(xp[:, c], taps[p], "valid")
    return u


def truepeak64(x, n_emitted):
    """max |u_c[4n + p]| over c, p and n < n_emitted, in float64 (0 for none):
    n_emitted = len(x) for a flushed stream, max(len(x) - 6, 0) without."""
    u = oversample64(x)[:max(int(n_emitted), 0)]
    return float(np.abs(u).max(initial=0.0))


def gain64(lufs, tp, target, max_dbtp):
    """The gain rule in float64, rounded to float32; tp None: no limit."""
    lufs = float(lufs)
    if not math.isfinite(lufs):
        return np.float32(1.0)
    g = 10.0 ** ((target - lufs) / 20.0)
    if tp is not None:
        c = 10.0 ** (max_dbtp / 20.0)
        if float(tp) > 0.0 and g * float(tp) > c:
            g = c / float(tp)
    return np.float32(g)


def int16_of(y):
    """The packed sink's int16 conversion: clip(floor(float64(y) * 32768 + 0.5))."""
    v = np.floor(np.asarray(y, np.float32).astype(np.float64) * 32768.0 + 0.5)
    return np.clip(v, -32768.0, 32767.0).astype(np.int16)


# ---- the filter ------------------------------------------------------------------
def test_filter_is_the_formula():
    got = mp3_amd.truepeak_filter()
    assert got.dtype == np.float32 and got.shape == (R, T)
    assert np.array_equal(got.view(np.uint32), taps64().view(np.uint32))


def test_filter_structure():
    taps = mp3_amd.truepeak_filter()
    delta = np.zeros(T, np.float32)
    delta[PRE] = 1.0
    assert np.array_equal(taps[0].view(np.uint32), delta.view(np.uint32))  # row 0 is exactly the delta
    # rows 1 and 3 mirror each other (tap 11 - j of phase 3 sits at -t of tap j of phase 1), row 2 itself
    assert np.array_equal(taps[1, ::-1], taps[3])
    assert np.array_equal(taps[2], taps[2, ::-1])
    for p in range(R):
        assert abs(taps[p].astype(np.float64).sum() - 1.0) <= 2.0 ** -22, p
    assert np.abs(taps.astype(np.float64)).sum(1).max() < 1.86


def test_filter_facts():
    """The three figures DESIGN.md section 4f quotes, computed here in float64."""
    taps = taps64().astype(np.float64)
    l1 = np.abs(taps).sum(1).max()
    n = np.arange(4096)
    sine = np.sin(2.0 * np.pi * 0.25 * n + np.pi / 4.0).astype(np.float32)[:, None]
    assert abs(np.abs(sine).max() - math.sqrt(0.5)) < 1e-6
    reads = truepeak64(sine, len(sine))
    # a steady sine at f (in units of fs) leaves phase p scaled by |H_p(f)|: the under-read of that phase
    j = np.arange(T)

    def under_read(fmax):
        f = np.linspace(0.0, fmax, 701)[:, None, None]
        H = np.abs((taps[None] * np.exp(-2j * np.pi * f * j)).sum(2))
        return float((-20.0 * np.log10(H)).max())

    w30, w33, w35 = under_read(0.30), under_read(0.33), under_read(0.35)
    print("max_p sum|taps| %.4f, fs/4 sine at 45 degrees reads %.4f, worst under-read of a phase: %.4f dB to 0.30 fs, "
          "%.4f dB to 0.33 fs, %.4f dB to 0.35 fs" % (l1, reads, w30, w33, w35))
    assert abs(l1 - 1.856) < 5e-4
    assert abs(reads - 1.013) < 5e-4
    assert w30 < 0.006 and w33 < 0.006 and 0.03 < w35 < 0.06


def test_reference_helpers():
    x = np.zeros((20, 2), np.float32)
    x[0, 0], x[5, 1] = 1.0, -1.0
    assert truepeak64(x, 20) == 1.0 and truepeak64(x, 0) == 0.0 and truepeak64(x[:0], 0) == 0.0
    u = oversample64(x)
    assert np.array_equal(u[:, 0, :], x.astype(np.float64))  # phase 0 reproduces x
    assert u[0, 1, 0] == float(taps64()[1, PRE]) and u[4, 1, 1] == -float(taps64()[1, PRE + 1])
    assert gain64(-np.inf, 1.0, -23.0, -1.0) == 1.0 and gain64(np.nan, 1.0, -23.0, -1.0) == 1.0
    assert gain64(-23.0, None, -23.0, -1.0) == 1.0
    assert gain64(-33.0, 1.0, -23.0, -1.0) == np.float32(10.0 ** (-1.0 / 20.0))  # the limit acts
    assert list(int16_of(np.array([0.5 / 32768, -0.5 / 32768, 1.5 / 32768, 2.0, -2.0, 0.99999], np.float32))) == \
        [1, 0, 2, 32767, -32768, 32767]


def test_argument_errors_and_exports():
    L = mp3_amd.lib()
    for name in NEW:
        assert name in mp3_amd.EXPORTS and hasattr(L, name), name
    assert L.mp3d_truepeak_filter(None, 0) == R * T  # size only
    buf = np.zeros(R * T, np.float32)
    assert L.mp3d_truepeak_filter(buf.ctypes.data, R * T - 1) == -1
    assert L.mp3d_truepeak_filter(buf.ctypes.data, R * T) == R * T
    assert L.mp3d_batch_set_true_peak(None, 1) == -1
    assert L.mp3d_batch_true_peak_time(None, None) == -1
    assert L.mp3d_batch_normalize_gain(None, None, None, 1, ctypes.c_double(-23.0), ctypes.c_double(-1.0), None,
                                       None) == -1
    assert L.mp3d_abi_version() == 5
