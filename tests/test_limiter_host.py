"""CPU: the limiter's definition (include/mp3d.h "limiter") restated in numpy,
the two host-only exports, and the properties the definition implies.

limit_ref is the reference of tests/test_gpu_limiter.py.  Its fmaf is exact:
the product of two float32 is exact in float64, the sum with the accumulator is
rounded to odd in float64 (the error term of the addition decides the last
bit) and then to float32, which cannot double-round (53 >= 2 * 24 + 2);
test_fma_is_libms checks it against libm's fmaf.  Everything after the
detector is float32 operations rounded once by numpy, or integers.
Everything here compares exactly: the definition has one value.
"""
import ctypes
import ctypes.util
import re

import numpy as np
import pytest

import mp3_amd
from mp3_amd import _build

FORMATS = [(48000, 2), (8000, 1), (11025, 2), (44100, 1)]
Q = 1 << 20


def look(fs):
    return (fs + 50) // 100


def ceiling(db):
    return np.float32(10.0 ** (db / 20.0))


def fma32(a, b, c):
    """fl32(a * b + c) of float32 arrays with one rounding"""
    p = a.astype(np.float64) * b.astype(np.float64)  # exact
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # s + err == p + c exactly
    bits = s.view(np.int64).copy()
    fix = (err != 0.0) & ((bits & 1) == 0)  # an inexact even sum: its odd neighbour on the error's side
    up = (err > 0.0) == (s > 0.0)  # away from zero
    bits += np.where(fix, np.where(up, 1, -1), 0)
    return bits.view(np.float64).astype(np.float32)


def detector(v):
    """p[i] of float32 v [n, ch]"""
    n, ch = v.shape
    taps = mp3_amd.truepeak_filter()
    pad = np.concatenate([np.zeros((5, ch), np.float32), v, np.zeros((6, ch), np.float32)])
    p = np.abs(v).max(axis=1) if n else np.zeros(0, np.float32)
    for ph in (1, 2, 3):
        acc = np.zeros((n, ch), np.float32)
        for j in range(12):
            acc = fma32(np.full((n, ch), taps[ph, j], np.float32), pad[j:j + n], acc)
        if n:
            p = np.maximum(p, np.abs(acc).max(axis=1))
    return p.astype(np.float32)


def limit_ref(x, fs, ceiling_db=-1.0, gain=None):
    """The definition on a whole stream x float32 [n, ch]: (y, g, r, v), g and
    r float32 [n]."""
    x = np.ascontiguousarray(x, np.float32)
    n, ch = x.shape
    A, c = look(fs), ceiling(ceiling_db)
    v = x if gain is None else x * np.float32(gain)
    p = detector(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(p <= c, np.float32(1.0), c / np.where(p <= c, np.float32(1.0), p)).astype(np.float32)
    R = np.floor(r * np.float32(1048576.0)).astype(np.int64)
    Rp = np.concatenate([np.full(3 * A, Q, np.int64), R, np.full(A, Q, np.int64)])
    m = np.lib.stride_tricks.sliding_window_view(Rp, 3 * A + 1).min(axis=1)  # m[k], k = -A .. n - 1
    cs = np.concatenate([[0], np.cumsum(m)])
    S = cs[A + 1:] - cs[:n]  # m[i - A .. i]
    assert len(S) == n and (S < 2 ** 31).all()
    G = S // (A + 1)
    g = G.astype(np.float32) * np.float32(2.0 ** -20)
    y = v * g[:, None]
    return y.astype(np.float32), g, r, v


def int16_of(y):
    """the packed sink's clamp(floor(y * 32768 + 0.5)) of float32 y"""
    v = np.asarray(y, np.float32) * np.float32(32768.0)  # exact
    f = np.floor(v)
    r = np.where(v - f >= np.float32(0.5), f + np.float32(1.0), f)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16)


def test_fma_is_libms():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(1)
    n = 100000
    a = (rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-12, 4, n)).astype(np.float32)
    b = (rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-12, 4, n)).astype(np.float32)
    c = (rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-12, 4, n)).astype(np.float32)
    # halfway cases of the float32 rounding, where a float64 sum rounded twice goes wrong
    # c in [1, 2) plus a product just under half an ulp of c, (1 + x 2^-23)(1 - x 2^-23) 2^-24: a float64 sum rounds
    # it up to the tie, which then goes to even
    k = n // 4
    xs = rng.integers(1, 300, k).astype(np.float64)
    c[:k] = rng.uniform(1.0, 2.0, k).astype(np.float32)
    a[:k] = ((1.0 + xs * 2.0 ** -23) * 2.0 ** -24).astype(np.float32)
    b[:k] = (1.0 - xs * 2.0 ** -23).astype(np.float32)
    want = np.array([libm.fmaf(float(p), float(q), float(s)) for p, q, s in zip(a, b, c)], np.float32)
    got = fma32(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    print("float64 sum rounded twice differs from fmaf in %d of %d" % ((twice != want).sum(), n))
    assert (twice != want).sum() > k // 4  # the triples do tell the two apart


def signal(fs, ch, n, kind, seed=0):
    rng = np.random.default_rng(seed + fs + ch)
    t = np.arange(n)
    if kind == "quiet":
        x = 0.5 * rng.uniform(-1.0, 1.0, (n, ch))
    elif kind == "noise":
        x = rng.uniform(-2.0, 2.0, (n, ch))
    else:  # a 440 Hz sine at 0.5 with a 4x burst
        x = np.repeat((0.5 * np.sin(2.0 * np.pi * 440.0 * t / fs))[:, None], ch, 1)
        x[n // 3: n // 3 + n // 10] *= 4.0
        if ch == 2:
            x[:, 1] *= 0.75
    return x.astype(np.float32)


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_properties(fs, ch):
    A = look(fs)
    n = 9 * A + 7
    for db in (-1.0, 0.0, -6.0):
        c = ceiling(db)
        bound = np.float64(c) * (1.0 + 2.0 ** -22)
        for kind in ("noise", "burst"):
            x = signal(fs, ch, n, kind)
            y, g, r, v = limit_ref(x, fs, db)
            assert y.shape == x.shape  # as many samples out as in
            assert (g <= r).all(), (db, kind)
            assert np.abs(y).astype(np.float64).max() <= bound, (db, kind)
            assert g.min() < 1.0
        x = signal(fs, ch, n, "quiet")
        x *= np.float32(0.5) * c
        assert detector(x).max() <= c
        y, g, r, v = limit_ref(x, fs, db)
        assert (g == 1.0).all() and np.array_equal(y.view(np.uint32), x.view(np.uint32))  # bit-identical


def test_envelope_shape():
    """One impulse: the gain falls linearly over the A samples before it, holds for Hd and releases over A + 1."""
    fs = 8000
    A = look(fs)
    i0, n = 5 * A, 12 * A
    x = np.zeros((n, 1), np.float32)
    x[i0] = 4.0
    y, g, r, v = limit_ref(x, fs, 0.0)
    G = np.round(g.astype(np.float64) * Q).astype(np.int64)
    lo = G.min()
    # R dips on the 12 indices whose chain sees the impulse, lowest at i0: m is lo on [i0 - A, i0 + 2A]
    assert (G[i0: i0 + 2 * A + 1] == lo).all() and lo == Q // 4
    assert (G[: i0 - 2 * A - 6] == Q).all() and (G[i0 + 3 * A + 1 + 6:] == Q).all()
    assert (np.diff(G[i0 - 2 * A - 6: i0 + 1]) <= 0).all() and (np.diff(G[i0 + 2 * A: i0 + 3 * A + 8]) >= 0).all()
    assert abs(float(y[i0, 0])) <= 1.0


def test_pre_gain_is_one_multiply():
    fs, ch = 11025, 2
    x = signal(fs, ch, 700, "noise")
    y, g, r, v = limit_ref(x, fs, -1.0, gain=3.0)
    assert np.array_equal(v, x * np.float32(3.0))
    y1, g1, _, v1 = limit_ref(x, fs, -1.0, gain=1.0)
    y0, g0, _, v0 = limit_ref(x, fs, -1.0)
    assert np.array_equal(y1.view(np.uint32), y0.view(np.uint32)) and v0 is not None


def test_lookahead_and_max_samples():
    want = {48000: 480, 8000: 80, 11025: 110, 22050: 221, 44100: 441}
    for fs in mp3_amd.RATES:
        A = mp3_amd.limiter_lookahead(fs)
        assert A == look(fs) == want.get(fs, A)
        for S in (0, 1, 1152, 2 ** 31 - 1):
            assert mp3_amd.limiter_max_samples(fs, S) == S + A + 6
    L = mp3_amd.lib()
    assert L.mp3d_limiter_lookahead(47999) == -1 and L.mp3d_limiter_lookahead(0) == -1
    assert L.mp3d_limiter_max_samples(47999, 10) == -1 and L.mp3d_limiter_max_samples(48000, -1) == -1
    assert L.mp3d_limiter_max_samples(48000, 2 ** 31) == -1
    with pytest.raises(mp3_amd.MP3DError):
        mp3_amd.limiter_lookahead(1234)


def test_header_declares_the_symbols():
    hdr = (_build.ROOT / "include" / "mp3d.h").read_text()
    for name in ("mp3d_limiter_lookahead", "mp3d_limiter_max_samples", "mp3d_batch_set_limiter", "mp3d_batch_limit",
                 "mp3d_batch_decode_limited", "mp3d_batch_limiter_time"):
        assert re.search(r"^MP3D_API [a-z ]+\b%s\(" % name, hdr, re.M), name
        assert name in mp3_amd.EXPORTS and hasattr(mp3_amd.lib(), name)
    assert re.search(r"^#define MP3D_ABI_VERSION 5$", hdr, re.M)
    L = mp3_amd.lib()
    assert L.mp3d_limiter_lookahead.restype is ctypes.c_longlong and L.mp3d_limiter_max_samples.restype is ctypes.c_longlong


def test_tile_budget():
    """The tile's span and integer array as mp3d_limiter.h states them."""
    h = (_build.CSRC / "mp3d_limiter.h").read_text()
    d = {k: int(v) for k, v in re.findall(r"^#define (MP3D_LIM_[A-Z]+)\s+(\d+)\b", h, re.M)}
    tile, amax = d["MP3D_LIM_TILE"], d["MP3D_LIM_AMAX"]
    assert amax == look(48000) and d["MP3D_LIM_Q"] == Q
    nr = d["MP3D_LIM_THREADS"] * d["MP3D_LIM_RSEG"]
    assert nr >= tile + 4 * amax and d["MP3D_LIM_THREADS"] * 16 >= tile + 4 * amax  # one round of chains
    assert d["MP3D_LIM_THREADS"] * d["MP3D_LIM_PSEG"] >= tile + amax
    assert 4 * amax + 11 == 1931
    runs = -(-(tile + 1931) // 16)
    assert nr // 16 >= -(-(tile + amax) // 16) + 3 * amax // 16 + 1  # the runs a thread with minima reads
    # k_lim_tile's arrays as declared: sx, ra, dbl[2], wtot and wmin
    waves = d["MP3D_LIM_THREADS"] // 64
    words = (nr // 16 + 1) * 17 + 2 * (d["MP3D_LIM_THREADS"] + 32) + 2 * waves
    for ch, stated in ((2, "80 828"), (1, "55 192")):
        lds = runs * 17 * ch * 4 + words * 4
        assert "{:,}".format(lds).replace(",", " ") == stated and stated + " bytes of arrays" in h
    lds = runs * 17 * 2 * 4 + words * 4
    assert 2 * (lds + 64) <= 160 * 1024  # two workgroups on a compute unit's 160 KB, alignment padding included
