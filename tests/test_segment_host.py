"""Host side of the segment sink (include/mp3d.h "segment sink"; no GPU
needed): the definition in numpy, its properties, the two host exports, and
the margins of the keypress fixture.

segments_ref restates the header.  Everything after the int16 quantisation is
integer arithmetic, so the GPU tests (tests/test_gpu_segment.py) compare with
it exactly.

On the look-ahead: the header's emit rule takes o[b] as final once
b <= B - S - P, a look-ahead of S - 1 + P hops.  The masks themselves need one
hop less: c[b] reads a[b - P + 1 .. b + P - 1] (with i < b < j and j - i <= P
both lie within P - 1 of b), so o[b] reads a[b - (S + P - 2) .. b + (S + P - 2)].
test_the_decided_prefix_is_stable checks all three statements: S - 1 + P is
enough (the rule), S - 2 + P is enough too (over every mask of up to 12 hops,
so no example to the contrary exists), S - 3 + P is not (an example).  The rule
is a definition and stays as the header states it: a segment comes out one hop
later than it could.
"""
import itertools

import numpy as np
import pytest

import _golden
import mp3_amd
from test_limiter_host import int16_of

MAXHOPS = 256


def hop(fs):
    return (fs + 50) // 100


# ---- the definition ---------------------------------------------------------------
def quantise(x):
    """q of float32 [n, ch]: the packed sink's int16 of the tempo sink's mono mix, as int64"""
    x = np.asarray(x, np.float32)
    m = x[:, 0] if x.shape[1] == 1 else np.float32(0.5) * (x[:, 0] + x[:, 1])
    return int16_of(m).astype(np.int64)


def hop_energy(q, H, flush):
    """E[0 .. B) of the quantised samples: B = floor(N / H), at a flush ceil(N / H) with zeros behind N"""
    N = len(q)
    B = -(-N // H) if flush else N // H
    sq = np.zeros(B * H, np.int64)
    sq[: min(N, B * H)] = (q * q)[: B * H]
    return sq.reshape(B, H).sum(axis=1)


def masks_windows(a, P, S):
    """(c, o) of the header, as it states them: c[b] by the nearest active hops on either side of b (the best i
    and j), o[b] by the windows of S that hold b"""
    a = np.asarray(a, bool)
    B = len(a)
    idx = np.arange(B)
    prev = np.maximum.accumulate(np.where(a, idx, -10 ** 9))  # the last i <= b with a[i]
    nxt = np.minimum.accumulate(np.where(a, idx, 10 ** 9)[::-1])[::-1]  # the first j >= b with a[j]
    c = nxt - prev <= P
    cs = np.concatenate([[0], np.cumsum(c)])
    e = np.zeros(B, bool)  # e[t]: c[t .. t + S - 1] all 1, inside [0, B)
    if B >= S:
        e[: B - S + 1] = cs[S:] - cs[: B - S + 1] == S
    es = np.concatenate([np.zeros(S, np.int64), np.cumsum(e)])
    o = es[S:] - es[:B] > 0  # some t in [b - S + 1, b]
    return c, o


def runs(m):
    """the maximal runs of ones of a mask, [(b0, b1)]"""
    d = np.diff(np.concatenate([[0], np.asarray(m, np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def masks_runs(a, P, S):
    """the same by run lengths: fill the inner runs of zeros shorter than P, then drop the runs of ones shorter
    than S"""
    a = np.asarray(a, bool)
    c = a.copy()
    for b0, b1 in runs(~a):
        if b0 > 0 and b1 < len(a) and b1 - b0 < P:
            c[b0:b1] = True
    o = np.zeros(len(a), bool)
    for b0, b1 in runs(c):
        if b1 - b0 >= S:
            o[b0:b1] = True
    return c, o


def emitted(a, P, S, pad, H, N, flush):
    """the segments a slot has emitted once it knows a[0 .. B): every run of o at a flush, else those that ended at
    b1 <= B - S - P"""
    B = len(a)
    o = masks_windows(a, P, S)[1]
    return [(max(b0 - pad, 0) * H, min((b1 + pad) * H, N)) for b0, b1 in runs(o) if flush or b1 <= B - S - P]


def segments_ref(x, fs, thr, P, S, pad, flush):
    """The segments of float32 x [n, ch] fed to a fresh slot in one call, [(start, end)]."""
    H = hop(fs)
    a = hop_energy(quantise(x), H, flush) >= thr
    return emitted(a, P, S, pad, H, len(x), flush)


def segments_by_call(x, fs, thr, P, S, pad, cuts, flush):
    """The segments each call emits when x is fed in pieces that end at the sample counts `cuts` (ascending, the
    last one len(x)), the last call with `flush`: what is emitted after a call less what was before it."""
    H = hop(fs)
    q = quantise(x)
    out, have = [], 0
    for k, n in enumerate(cuts):
        fl = flush and k == len(cuts) - 1
        now = emitted(hop_energy(q[:n], H, fl) >= thr, P, S, pad, H, n, fl)
        out.append(now[have:])
        have = len(now)
    return out


# ---- properties -------------------------------------------------------------------
def random_mask(rng, B):
    a = rng.random(B) < rng.choice([0.1, 0.3, 0.5, 0.8])
    if B and rng.random() < 0.5:  # lumpier runs
        a = np.repeat(a[: (B + 2) // 3], 3)[:B]
    return a


def test_the_two_forms_agree_and_runs_are_long_and_apart():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        P, S, B = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(0, 70))
        a = random_mask(rng, B)
        c1, o1 = masks_windows(a, P, S)
        c2, o2 = masks_runs(a, P, S)
        assert np.array_equal(c1, c2) and np.array_equal(o1, o2), (a, P, S)
        r = runs(o1)
        assert all(b1 - b0 >= S for b0, b1 in r)
        assert all(y0 - x1 >= P for (_, x1), (y0, _) in zip(r, r[1:]))
        pad = P // 2  # the largest pad: padded segments never overlap
        seg = emitted(a, P, S, pad, 10, B * 10, True)
        assert all(s1 <= t0 for (_, s1), (t0, _) in zip(seg, seg[1:]))
        if a.any():  # leading and trailing silence is never filled
            assert not c1[: np.flatnonzero(a)[0]].any() and not c1[np.flatnonzero(a)[-1] + 1:].any()


def stable_with(a, P, S, L):
    """o of every prefix a[:Bp] agrees with o of a on the hops b < Bp - L"""
    o = masks_windows(a, P, S)[1]
    for Bp in range(len(a) + 1):
        k = max(Bp - L, 0)
        if not np.array_equal(masks_windows(a[:Bp], P, S)[1][:k], o[:k]):
            return False
    return True


def test_the_decided_prefix_is_stable():
    rng = np.random.default_rng(1)
    for _ in range(300):
        P, S, B = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(0, 60))
        assert stable_with(random_mask(rng, B), P, S, S - 1 + P)
    # every mask of up to 10 hops: the rule's look-ahead, and one hop less, are enough (the module docstring)
    for P, S in itertools.product((1, 2, 3), (1, 2, 3)):
        for B in range(11):
            for bits in itertools.product((False, True), repeat=B):
                a = np.array(bits, bool)
                assert stable_with(a, P, S, S - 1 + P) and stable_with(a, P, S, S - 2 + P), (bits, P, S)
    # two hops less are not: the far end of a pause of P - 1, and of a run of S
    assert not stable_with(np.array([1, 0, 0, 1], bool), 3, 1, 3 + 1 - 3)
    assert not stable_with(np.array([1, 1, 1], bool), 1, 3, 1 + 3 - 3)
    assert not stable_with(np.array([1, 0, 1, 0, 0, 1], bool), 3, 4, 3 + 4 - 3)


def test_segment_max_is_never_exceeded():
    """Brute force: every split of a random mask into two calls, flushed and not, with small P and S; the count of
    each call against mp3d_segment_max of its samples."""
    fs, H = 8000, 80
    rng = np.random.default_rng(2)
    worst = -10
    for _ in range(60):
        P, S = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        B = int(rng.integers(1, 40))
        a = random_mask(rng, B)
        tail = int(rng.integers(0, H))  # a part hop behind the last whole one (silent: E = 0 < thr)
        N = B * H + tail
        full = np.concatenate([a, [False]]) if tail else a
        # every split: at each hop edge and a sample to either side of it (the hops a call completes, and so what
        # it emits, change nowhere else)
        cuts = sorted({c for b in range(B + 2) for c in (b * H - 1, b * H, b * H + 1) if 0 <= c <= N})
        for n0 in cuts:
            for flush in (False, True):
                first = emitted(a[: n0 // H], P, S, 0, H, n0, False)
                Bn = -(-N // H) if flush else N // H
                both = emitted(full[:Bn], P, S, 0, H, N, flush)
                assert both[: len(first)] == first
                for got, fed in ((len(first), n0), (len(both) - len(first), N - n0)):
                    bound = mp3_amd.segment_max(fs, fed, P, S)
                    assert got <= bound, (a, P, S, n0, flush)
                    worst = max(worst, got - bound)
    assert worst >= -2  # (the bound is not idle: some call comes within two of it)


def test_segment_max_values_and_errors():
    for fs in mp3_amd.RATES:
        H = hop(fs)
        for n, P, S in [(0, 1, 1), (1, 1, 1), (H, 30, 10), (10 * H + 1, 5, 3), (2 ** 31 - 1, 256, 256), (12345, 1, 256)]:
            K = -(-(n + H - 1) // H)
            assert mp3_amd.segment_max(fs, n, P, S) == 2 + K // (S + P)
    L = mp3_amd.lib()
    assert L.mp3d_segment_max(44100, 100, 30, 10) > 0
    for args in [(44000, 100, 30, 10), (44100, -1, 30, 10), (44100, 2 ** 31, 30, 10), (44100, 100, 0, 10),
                 (44100, 100, 257, 10), (44100, 100, 30, 0), (44100, 100, 30, 257)]:
        assert L.mp3d_segment_max(*args) == -1, args


def test_segment_threshold_values_and_errors():
    for fs in mp3_amd.RATES:
        H = hop(fs)
        assert mp3_amd.segment_threshold(fs, 0.0) == H * 2 ** 30  # the largest hop energy there is
        for db in (-96.0, -60.0, -40.0, -23.5, -6.0, -0.001):
            want = max(1.0, np.ceil(H * 2.0 ** 30 * 10.0 ** (db / 10.0)))
            assert abs(mp3_amd.segment_threshold(fs, db) - int(want)) <= 1, (fs, db)
        assert mp3_amd.segment_threshold(fs, -96.0) >= 1
    L = mp3_amd.lib()
    for args in [(44000, -40.0), (0, -40.0), (44100, 0.001), (44100, -96.001), (44100, float("nan")),
                 (44100, float("inf")), (44100, float("-inf"))]:
        assert L.mp3d_segment_threshold(*args) == -1, args


# ---- the keypress fixture ---------------------------------------------------------
def keypress():
    """the tagged keypress stream's gapless PCM as float32 [n, 2] (int16 / 32768: q gives the int16 back)"""
    pcm = np.load(_golden.GOLDEN / "keypress_128k_js.tagged.pcm16.npy")
    pcm = pcm if pcm.shape[-1] == 2 else pcm.T
    return pcm.astype(np.float32) / np.float32(32768.0)


def test_keypress_margins():
    """Every hop of the fixture at 44.1 kHz is on its side of -40 dBFS by more than a decoder that differs by one
    LSB in every sample could move it: E - d >= thr or E + d < thr with d = sum (2 |q| + 1).  So the GPU test on
    the decoded file (tests/test_gpu_segment.py) can expect the list computed here from the fixture."""
    fs, H = 44100, 441
    thr = mp3_amd.segment_threshold(fs, -40.0)
    assert thr == 47352015
    q = quantise(keypress())
    B = -(-len(q) // H)
    E = hop_energy(q, H, True)
    qq = np.zeros(B * H, np.int64)
    qq[: len(q)] = np.abs(q)
    d = (2 * qq + 1).reshape(B, H).sum(axis=1)
    a = E >= thr
    assert np.all(np.where(a, E - d >= thr, E + d < thr))
    assert B == 53 and a[:20].all() and not a[20:].any()
    assert (int(E[20]), int(d[20])) == (45172229, 251647)  # the nearest
    assert E.max() > 2 ** 32 and 3.3e10 < E.max() < 3.5e10  # a 32-bit sum would not hold it
    assert segments_ref(keypress(), fs, thr, 5, 3, 2, True) == [(0, 9702)]
