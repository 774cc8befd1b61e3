"""The equaliser sink's definition and numerical contract in numpy (include/mp3d.h
"equaliser sink"): the reference of tests/test_eq_host.py
and tests/test_gpu_eq.py.

    design_ld        the cookbook sections in np.longdouble, unrounded
    seq              the definition, sample by sample, in float64 or longdouble
    par64            a float64 restatement of the kernels' time-parallel form
                     with the header's tile and segment sizes
    curves, signals, LENGTHS, FORMATS    the test list
    bound, EPS       |y - ref| <= 2^-22 |ref| + EPS G,  G the running peak of |ref|

EPS is 4 x the largest |y - ref| / G that par64 (in float64, before the
rounding to float32) reaches against seq in np.longdouble over every format,
curve, signal and length below, measured on the CPU; tests/test_eq_host.py
asserts it at EPS / 4.  The factor 4 covers the kernels' fused multiply-adds
and their other order inside a matrix row.  The constant never comes from what
the GPU returns.  The contract caps it: EPS <= 2^-26, a quarter of a float32
half-ulp at the peak.
"""
import functools
import pathlib
import re

import numpy as np

HDR = (pathlib.Path(__file__).resolve().parents[1] / "mp3_amd" / "csrc" / "mp3d_eq.h").read_text()
SEG = int(re.search(r"#define MP3D_EQ_SEG (\d+)", HDR).group(1))
TILE = int(re.search(r"#define MP3D_EQ_TILE (\d+)", HDR).group(1))
THREADS = TILE // SEG
WAVES = THREADS // 64
MAX_BANDS = 10
PEAK, LOW_SHELF, HIGH_SHELF, HIGH_PASS, LOW_PASS = range(5)

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))

# Measured: the largest |par64 - seq longdouble| / G over the whole test list is
# 3.27e-11 (curve 1 at 44.1 kHz, the DC step, TILE - 1 samples); rounded up to
# two digits.
EPS_MEASURED = 3.3e-11
EPS = 4 * EPS_MEASURED
EPS_CAP = 2.0 ** -26

FORMATS = [(48000, 2), (44100, 2), (11025, 1), (8000, 1)]
LENGTHS = [0, 1, SEG - 1, SEG, SEG + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
SIGNALS = ["impulse", "sine997", "noise", "dc_step", "quiet_after_loud"]
CURVES = ["pole20", "graphic", "five_types", "flat"]


# ---- design -------------------------------------------------------------------------
def design_ld(hz, bands, preamp_db=0.0):
    """longdouble [K, 5]: b0 b1 b2 a1 a2 of each stage, a0 = 1, preamp on stage 1"""
    out = np.zeros((len(bands), 5), LD)
    for k, (typ, f0, gain_db, q) in enumerate(bands):
        w0 = LD(2) * PI * LD(f0) / LD(hz)
        cs, alpha = np.cos(w0), np.sin(w0) / (LD(2) * LD(q))
        A = LD(10) ** (LD(gain_db) / LD(40))
        sq = LD(2) * np.sqrt(A) * alpha
        one, two = LD(1), LD(2)
        if typ == PEAK:
            b = [one + alpha * A, -two * cs, one - alpha * A]
            a = [one + alpha / A, -two * cs, one - alpha / A]
        elif typ == LOW_SHELF:
            b = [A * ((A + one) - (A - one) * cs + sq), two * A * ((A - one) - (A + one) * cs),
                 A * ((A + one) - (A - one) * cs - sq)]
            a = [(A + one) + (A - one) * cs + sq, -two * ((A - one) + (A + one) * cs), (A + one) + (A - one) * cs - sq]
        elif typ == HIGH_SHELF:
            b = [A * ((A + one) + (A - one) * cs + sq), -two * A * ((A - one) + (A + one) * cs),
                 A * ((A + one) + (A - one) * cs - sq)]
            a = [(A + one) - (A - one) * cs + sq, two * ((A - one) - (A + one) * cs), (A + one) - (A - one) * cs - sq]
        elif typ == HIGH_PASS:
            b = [(one + cs) / two, -(one + cs), (one + cs) / two]
            a = [one + alpha, -two * cs, one - alpha]
        elif typ == LOW_PASS:
            b = [(one - cs) / two, one - cs, (one - cs) / two]
            a = [one + alpha, -two * cs, one - alpha]
        else:
            raise ValueError(typ)
        g = LD(10) ** (LD(preamp_db) / LD(20)) if k == 0 else one
        out[k] = [b[0] * g / a[0], b[1] * g / a[0], b[2] * g / a[0], a[1] / a[0], a[2] / a[0]]
    return out


def design64(hz, bands, preamp_db=0.0):
    """... rounded once to double: what mp3d_eq_design returns"""
    return design_ld(hz, bands, preamp_db).astype(np.float64)


def response_db(coef, f, hz):
    """|H| in dB of the cascade coef [K, 5] at frequency f, in longdouble"""
    w = LD(2) * PI * LD(f) / LD(hz)
    z1 = np.cos(w) - 1j * np.sin(w).astype(np.clongdouble)
    h = np.clongdouble(1)
    for b0, b1, b2, a1, a2 in np.asarray(coef, LD):
        h = h * (b0 + b1 * z1 + b2 * z1 * z1) / (LD(1) + a1 * z1 + a2 * z1 * z1)
    return LD(20) * np.log10(np.abs(h))


# ---- the definition, sequentially -----------------------------------------------------
def seq(coef, x, dt=np.float64):
    """x [T] or [T, L] (time first; float32 values) through the cascade coef
    [K, 5] (or [K, 5, L]: a curve per lane) from a zero state, every operation
    in dt, sample by sample: o = b0 v + s1; s1 = b1 v - a1 o + s2; s2 = b2 v -
    a2 o.  The stages run as a systolic array (stage k is at sample i - k in
    step i), which changes no operation and no operand."""
    x = np.asarray(x)
    flat = x.ndim == 1
    x = (x[:, None] if flat else x).astype(dt)
    T, L = x.shape
    c = np.asarray(coef).astype(dt)
    K = c.shape[0]
    c = c[:, :, None] if c.ndim == 2 else c
    b0, b1, b2, a1, a2 = (np.ascontiguousarray(np.broadcast_to(c[:, i], (K, L))) for i in range(5))
    s1, s2, u = np.zeros((K, L), dt), np.zeros((K, L), dt), np.zeros((K, L), dt)
    y = np.zeros((T, L), dt)
    for i in range(T + K - 1):
        u[0] = x[i] if i < T else 0
        o = b0 * u + s1
        s1 = b1 * u - a1 * o + s2
        s2 = b2 * u - a2 * o
        if i >= K - 1:
            y[i - K + 1] = o[K - 1]
        u[1:] = o[:-1]
    return y[:, 0] if flat else y


# ---- the time-parallel form, restated in float64 ---------------------------------------
def _matpow_tables(coef):
    """(apow [K, 65, 2, 2], tpow [65, 2K, 2K]) as mp3d_eq.cpp builds them: in
    longdouble from the double coefficients, rounded to double"""
    c = np.asarray(coef, np.float64).astype(LD)
    K = len(c)
    apow = np.zeros((K, 65, 2, 2))
    for k in range(K):
        seg = np.array([[-c[k, 3], LD(1)], [-c[k, 4], LD(0)]], LD)
        for _ in range(int(np.log2(SEG))):
            seg = seg @ seg
        p = np.eye(2, dtype=LD)
        for d in range(65):
            apow[k, d] = p.astype(np.float64)
            p = p @ seg
    n = 2 * K
    A = np.zeros((n, n), LD)
    for j in range(n):
        u = LD(0)
        for k in range(K):
            s1, s2 = LD(2 * k == j), LD(2 * k + 1 == j)
            o = c[k, 0] * u + s1
            A[2 * k, j] = c[k, 1] * u - c[k, 3] * o + s2
            A[2 * k + 1, j] = c[k, 2] * u - c[k, 4] * o
            u = o
    for _ in range(int(np.log2(TILE))):
        A = A @ A
    tpow = np.zeros((65, n, n))
    q = np.eye(n, dtype=LD)
    for d in range(65):
        tpow[d] = q.astype(np.float64)
        q = q @ A
    return apow, tpow


def _tile_pass(coef, apow, v, entry, cnt, f32_state):
    """k_eq_local / k_eq_apply: v [L, T, THREADS, SEG], entry [L, T, 2K], cnt
    [T, THREADS] -> (outputs like v, every thread's end state [L, T, THREADS, 2K])"""
    L, T = v.shape[:2]
    K = len(coef)
    v = v.copy()
    ends = np.zeros((L, T, THREADS, 2 * K))
    keep = [(i < cnt)[None] for i in range(SEG)]
    rnd = (lambda s: s.astype(np.float32).astype(np.float64)) if f32_state else (lambda s: s)

    def run(s1, s2, store):
        for i in range(SEG):
            x = v[..., i]
            o = b0 * x + s1
            s1 = np.where(keep[i], rnd(b1 * x - a1 * o + s2), s1)
            s2 = np.where(keep[i], rnd(b2 * x - a2 * o), s2)
            if store:
                v[..., i] = o
        return s1, s2

    for k in range(K):
        b0, b1, b2, a1, a2 = (float(t) for t in coef[k])
        z1, z2 = run(np.zeros((L, T, THREADS)), np.zeros((L, T, THREADS)), False)
        z = np.stack([z1, z2], -1).reshape(L, T, WAVES, 64, 2)
        d = 1
        while d < 64:  # the scan over a wave's lanes
            z[..., d:, :] = z[..., d:, :] + z[..., :-d, :] @ apow[k, d].T
            d *= 2
        E, Ew = entry[..., 2 * k:2 * k + 2], []
        for w in range(WAVES):  # the walk over the waves' totals
            Ew.append(E)
            E = E @ apow[k, 64].T + z[:, :, w, 63]
        Ew = np.stack(Ew, 2)  # [L, T, WAVES, 2]
        f = np.concatenate([np.zeros_like(z[..., :1, :]), z[..., :-1, :]], -2)
        f = f + np.einsum("nij,ltwj->ltwni", apow[k, :64], Ew)
        f = rnd(f).reshape(L, T, THREADS, 2)
        e1, e2 = run(f[..., 0], f[..., 1], True)
        ends[..., 2 * k], ends[..., 2 * k + 1] = e1, e2
    return v, ends


def par64(coef, x, defect=None):
    """x [L, N] (float32 values) through the cascade coef [K, 5] from a zero
    state as one call of the kernels computes it, in float64 and before the
    rounding to float32: y [L, N].  defect seeds an implementation mistake:
    "f32_state", "shift" (every tile but the first starts a sample late),
    "no_carry" (every tile but the first starts from a zero state)."""
    coef = np.asarray(coef, np.float64)
    x = np.asarray(x, np.float64)
    L, N = x.shape
    K = len(coef)
    if N == 0:
        return np.zeros((L, 0))
    T = -(-N // TILE)
    apow, tpow = _matpow_tables(coef)
    xp = np.zeros((L, T * TILE + 1))
    xp[:, :N] = x
    tiles = xp[:, :T * TILE].reshape(L, T, TILE).copy()
    if defect == "shift":
        tiles[:, 1:] = xp[:, 1:].reshape(L, T, TILE)[:, 1:]
    v = tiles.reshape(L, T, THREADS, SEG)
    start = np.arange(T)[:, None] * TILE + np.arange(THREADS)[None, :] * SEG
    cnt = np.clip(N - start, 0, SEG)
    f32 = defect == "f32_state"
    entry = np.zeros((L, T, 2 * K))
    if T > 1:
        # k_eq_local: z of every tile another follows
        _, ends = _tile_pass(coef, apow, v[:, :T - 1], np.zeros((L, T - 1, 2 * K)), np.full((T - 1, THREADS), SEG), f32)
        tz = ends[:, :, THREADS - 1]
        # k_eq_carry: 64 tiles per scan
        E = np.zeros((L, 2 * K))
        for base in range(0, T, 64):
            z = np.zeros((L, 64, 2 * K))
            m = max(0, min(64, T - 1 - base))
            z[:, :m] = tz[:, base:base + m]
            d = 1
            while d < 64:
                z[:, d:] = z[:, d:] + z[:, :-d] @ tpow[d].T
                d *= 2
            f = np.concatenate([np.zeros((L, 1, 2 * K)), z[:, :-1]], 1) + np.einsum("nij,lj->lni", tpow[:64], E)
            m = min(64, T - base)
            entry[:, base:base + m] = f[:, :m]
            E = z[:, 63] + E @ tpow[64].T
        if defect == "no_carry":
            entry[:, 1:] = 0.0
    y, _ = _tile_pass(coef, apow, v, entry, cnt, f32)
    return y.reshape(L, T * TILE)[:, :N]


# ---- the bound --------------------------------------------------------------------------
def bound(ref, eps=EPS):
    """per sample, ref [N] or [N, ...] with time first: 2^-22 |ref| + eps G"""
    a = np.abs(np.asarray(ref, np.float64))
    return 2.0 ** -22 * a + eps * np.maximum.accumulate(a, axis=0)


def excess(y, ref, eps=EPS):
    """the largest |y - ref| / bound (0 / 0 = 0; anything else over 0, or a NaN, is inf)"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    err, b = np.abs(y - ref), bound(ref, eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(np.inf if np.isnan(r).any() else r.max())


# ---- the test list ------------------------------------------------------------------------
def curve(name, hz):
    """(bands, preamp_db)"""
    if name == "pole20":  # the pole nearest the unit circle
        return [(PEAK, 20.0, 12.0, 16.0)], 0.0
    if name == "graphic":  # octave bands from 31.25 Hz under 0.45 fs, alternating +-12 dB
        f = [31.25 * 2 ** k for k in range(MAX_BANDS) if 31.25 * 2 ** k < 0.45 * hz]
        return [(PEAK, fk, 12.0 if k % 2 == 0 else -12.0, 1.41) for k, fk in enumerate(f)], -6.0
    if name == "five_types":
        return [(HIGH_PASS, 80.0, 0.0, 0.707), (LOW_SHELF, 200.0, 6.0, 0.707), (PEAK, 1000.0, -9.0, 4.0),
                (HIGH_SHELF, 0.3 * hz, -6.0, 0.707), (LOW_PASS, 0.4 * hz, 0.0, 0.707)], 0.0
    if name == "flat":
        return [(PEAK, 100.0, 0.0, 1.0), (PEAK, 1000.0, 0.0, 4.0), (PEAK, 3000.0, 0.0, 0.5)], 0.0
    raise ValueError(name)


def signal(name, hz, n, ch, seed=0):
    """float32 [n, ch]; the second channel is another signal of the same kind"""
    out = np.zeros((n, ch), np.float32)
    i = np.arange(n)
    for c in range(ch):
        rng = np.random.default_rng([CURVES.index("flat") + 7, SIGNALS.index(name), c, seed])
        if name == "impulse":
            if n > c:
                out[c, c] = 1.0  # (the second channel's a sample later)
        elif name == "sine997":
            out[:, c] = 0.5 * np.sin(2 * np.pi * 997.0 * i / hz + 0.7 * c)
        elif name == "noise":
            out[:, c] = rng.uniform(-1.0, 1.0, n)
        elif name == "dc_step":
            out[:, c] = 0.9 if c == 0 else -0.9
        elif name == "quiet_after_loud":
            out[:, c] = rng.uniform(-1.0, 1.0, n) * np.where(i < 2 * TILE, 1.0, 1e-4)
        else:
            raise ValueError(name)
    return out


@functools.lru_cache(maxsize=None)
def streams(hz, ch):
    """the ragged batch: every signal at every length, [(name, n, x float32 [n, ch])], read-only"""
    out = []
    for name in SIGNALS:
        for n in LENGTHS:
            x = signal(name, hz, n, ch)
            x.setflags(write=False)
            out.append((name, n, x))
    return out


def lanes(hz, ch):
    """the batch as seq's lanes: float32 [max n, streams * ch], zero past a stream's end"""
    st = streams(hz, ch)
    x = np.zeros((max(LENGTHS), len(st) * ch), np.float32)
    for s, (_, n, v) in enumerate(st):
        x[:n, s * ch:(s + 1) * ch] = v
    return x


@functools.lru_cache(maxsize=None)
def reference(hz, ch, name, dt=np.float64):
    """seq of the ragged batch under curve `name`: [(n, ref dt [n, ch])] per stream, read-only"""
    bands, pre = curve(name, hz)
    y = seq(design64(hz, bands, pre), lanes(hz, ch), dt)
    out = []
    for s, (_, n, _) in enumerate(streams(hz, ch)):
        r = y[:n, s * ch:(s + 1) * ch].copy()
        r.setflags(write=False)
        out.append((n, r))
    return out
