"""The host-only half of the loudness sink (include/mp3d.h "loudness sink"; no
GPU needed): the K-weighting coefficients against the BS.1770 table and a
float64 restatement of the header's formula, the stride bound against the emit
rule by brute force, the gated integrated loudness against its restatement,
the 997 Hz calibration anchor, argument errors and the exports.

The restatement below (coef64, kweight64, blocks64, integrated64) is also the
reference of tests/test_gpu_loudness.py."""
import ctypes
import math

import numpy as np
import pytest

import mp3_amd

try:
    from scipy.signal import lfilter
except Exception:  # the sample loop below does the same, slower
    lfilter = None

NEW = ["mp3d_batch_decode_loudness", "mp3d_batch_loudness", "mp3d_batch_loudness_integrated",
       "mp3d_batch_loudness_time", "mp3d_batch_set_loudness", "mp3d_loud_max_blocks", "mp3d_loudness_filter",
       "mp3d_loudness_integrated"]

TABLE_48K = [[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
             [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]]


# ---- the definition in float64 ---------------------------------------------------
def coef64(fs):
    """[[b0 b1 b2 a1 a2] of the shelf, of the high-pass] for the rate fs."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
          2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    s2 = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([s1, s2], np.float64)


def biquad64(v, c):
    """Transposed direct form II in float64 from a zero state."""
    v = np.asarray(v, np.float64)
    if lfilter is not None:
        return lfilter(c[:3], [1.0, c[3], c[4]], v)
    assert v.size <= 400000
    o = np.zeros(v.size)
    s1 = s2 = 0.0
    b0, b1, b2, a1, a2 = (float(x) for x in c)
    for i, x in enumerate(v.tolist()):
        y = b0 * x + s1
        s1 = b1 * x - a1 * y + s2
        s2 = b2 * x - a2 * y
        o[i] = y
    return o


def kweight64(x, c):
    """x [N] of one channel (float32 values) -> y float64 [N]."""
    return biquad64(biquad64(np.asarray(x, np.float32).astype(np.float64), c[0]), c[1])


def block_len(fs):
    return (fs + 5) // 10


def blocks64(x, fs, c=None):
    """x float32 [N, C] since the restart -> z float64 [N // H]."""
    x = np.asarray(x, np.float32)
    x = x[:, None] if x.ndim == 1 else x
    c = coef64(fs) if c is None else c
    H = block_len(fs)
    nb = x.shape[0] // H
    z = np.zeros(nb)
    for ch in range(x.shape[1]):
        y = kweight64(x[:, ch], c)[: nb * H]
        z += (y * y).reshape(nb, H).sum(axis=1) / H
    return z


def integrated64(z):
    z = np.asarray(z, np.float64)
    if z.size < 4:
        return -np.inf
    G = (z[:-3] + z[1:-2] + z[2:-1] + z[3:]) / 4.0
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(G)
    j1 = l > -70.0
    if not j1.any():
        return -np.inf
    gamma = -0.691 + 10.0 * np.log10(G[j1].mean()) - 10.0
    j2 = j1 & (l > gamma)
    if not j2.any():
        return -np.inf
    return float(-0.691 + 10.0 * np.log10(G[j2].mean()))


# ---- coefficients ----------------------------------------------------------------
def test_filter_at_48k_is_the_bs1770_table():
    c = mp3_amd.loudness_filter(48000)
    assert c.dtype == np.float64 and c.shape == (2, 5)
    assert np.abs(c - np.array(TABLE_48K)).max() <= 1e-12
    assert np.abs(coef64(48000) - np.array(TABLE_48K)).max() <= 1e-12  # (and so is the restatement)


@pytest.mark.parametrize("hz", [r for r in mp3_amd.RATES if r != 48000])
def test_filter_is_the_formula(hz):
    c, want = mp3_amd.loudness_filter(hz), coef64(hz)
    assert (np.abs(c - want) <= 1e-14 * np.abs(want)).all()


def test_filter_argument_errors():
    L = mp3_amd.lib()
    buf = np.zeros(10, np.float64)
    for hz in (0, 44000, 96000, -48000):
        assert L.mp3d_loudness_filter(hz, buf.ctypes.data, 10) == -1
    assert L.mp3d_loudness_filter(48000, None, 0) == 10
    assert L.mp3d_loudness_filter(48000, buf.ctypes.data, 9) == -1 and not buf.any()
    assert L.mp3d_loudness_filter(48000, buf.ctypes.data, 10) == 10 and buf.all()
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        mp3_amd.loudness_filter(22000)


# ---- the stride bound ------------------------------------------------------------
def test_block_lengths():
    assert [block_len(r) for r in mp3_amd.RATES] == [800, 1103, 1200, 1600, 2205, 2400, 3200, 4410, 4800]


@pytest.mark.parametrize("out_hz", mp3_amd.RATES)
@pytest.mark.parametrize("frames", [1, 3])
def test_loud_max_blocks(out_hz, frames):
    H = block_len(out_hz)
    r = np.arange(H, dtype=np.int64)[:, None]  # samples of the open block before the call
    for min_hz in mp3_amd.RATES:  # every input rate as the lowest one
        S = mp3_amd.packed_max_samples(out_hz, frames, min_hz)
        bound = mp3_amd.loud_max_blocks(out_hz, frames, min_hz)
        assert S > 0 and bound == (H - 1 + S) // H
        s = np.unique(np.concatenate([np.arange(min(S, 2 * H) + 1), np.arange(max(S - 2 * H, 0), S + 1),
                                      np.linspace(0, S, 257).astype(np.int64)]))[None, :]
        closed = (r + s) // H  # complete blocks of the call
        assert closed.max() <= bound  # never exceeded
        assert closed.max() >= bound - 1  # loose by at most 1
    assert mp3_amd.loud_max_blocks(out_hz, frames) == mp3_amd.loud_max_blocks(out_hz, frames, 8000)


def test_loud_max_blocks_edges():
    L = mp3_amd.lib()
    assert L.mp3d_loud_max_blocks(48000, 4, 48001) == 0  # no input rate that high: S = 0
    assert L.mp3d_loud_max_blocks(48000, -1, 8000) == -1
    assert L.mp3d_loud_max_blocks(47999, 4, 8000) == -1


# ---- integrated loudness ---------------------------------------------------------
def lib_integrated(z):
    z = np.ascontiguousarray(z, np.float32)
    got = mp3_amd.integrated_lufs(z)
    want = integrated64(z.astype(np.float64))
    if np.isinf(want):
        assert got == -np.inf
    else:
        assert abs(got - want) <= 1e-9, (got, want)
    return got


def test_integrated_constant():
    got = lib_integrated(np.full(50, 0.25, np.float32))
    assert abs(got - (-0.691 + 10.0 * math.log10(0.25))) <= 1e-9


def test_integrated_needs_four_blocks():
    assert lib_integrated(np.full(3, 0.5, np.float32)) == -np.inf
    assert lib_integrated(np.zeros(0, np.float32)) == -np.inf
    assert np.isfinite(lib_integrated(np.full(4, 0.5, np.float32)))


def test_integrated_all_below_the_absolute_gate():
    assert lib_integrated(np.full(40, 1e-8, np.float32)) == -np.inf  # -80.7 LUFS
    assert lib_integrated(np.zeros(40, np.float32)) == -np.inf


def test_integrated_relative_gate_cuts_the_quiet_part():
    z = np.concatenate([np.full(40, 1e-1, np.float32), np.full(40, 1e-4, np.float32)])
    got = lib_integrated(z)
    loud = -0.691 + 10.0 * math.log10(1e-1)
    ungated = -0.691 + 10.0 * math.log10(float(z.astype(np.float64).mean()))
    assert abs(got - loud) < 0.2 and got > ungated + 2.0  # the quiet half is gated out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_integrated_random(seed):
    rng = np.random.default_rng(seed)
    for n in (4, 5, 37, 600):
        lib_integrated((10.0 ** rng.uniform(-9.0, 0.0, n)).astype(np.float32))


def test_integrated_argument_errors():
    L = mp3_amd.lib()
    out = ctypes.c_double(1.0)
    z = np.ones(8, np.float32)
    assert L.mp3d_loudness_integrated(z.ctypes.data, 8, None) == -1
    assert L.mp3d_loudness_integrated(None, 8, ctypes.byref(out)) == -1
    assert L.mp3d_loudness_integrated(z.ctypes.data, -1, ctypes.byref(out)) == -1


# ---- calibration -----------------------------------------------------------------
ANCHOR = {48000: -3.0103, 44100: -3.0075, 16000: -2.9700, 11025: -2.9693, 8000: -2.9962}


@pytest.mark.parametrize("hz", sorted(ANCHOR))
def test_997_hz_full_scale_sine(hz):
    """3 s of a full-scale 997 Hz sine on one channel, filtered in float64
    with the library's coefficients: -3.01 LUFS at 48 kHz (BS.1770)."""
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * hz) / hz).astype(np.float32)
    z = blocks64(x, hz, mp3_amd.loudness_filter(hz))
    assert z.size == 3 * hz // block_len(hz)
    got = mp3_amd.integrated_lufs(z.astype(np.float32))
    assert abs(got - ANCHOR[hz]) <= 0.002, got
    assert abs(integrated64(z) - ANCHOR[hz]) <= 0.002


# ---- exports ---------------------------------------------------------------------
def test_exports():
    names = sorted(mp3_amd.EXPORTS)
    L = mp3_amd.lib()
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    assert L.mp3d_abi_version() == 5
    # a NULL handle is refused before anything touches a device
    f, i = ctypes.c_float(), ctypes.c_int()
    assert L.mp3d_batch_set_loudness(None, 1) == -1
    assert L.mp3d_batch_loudness(None, None, 0, ctypes.byref(i), 1, ctypes.byref(f), 1, ctypes.byref(i), None, 0,
                                 None) == -1
    assert L.mp3d_batch_decode_loudness(None, None, None, None, 1, 1, ctypes.byref(f), 1, ctypes.byref(i), None, 0, None,
                                        None) == -1
    assert L.mp3d_batch_loudness_integrated(None, ctypes.byref(f), 1, ctypes.byref(i), 1, ctypes.byref(f), None) == -1
    assert L.mp3d_batch_loudness_time(None, ctypes.byref(f)) == -1
