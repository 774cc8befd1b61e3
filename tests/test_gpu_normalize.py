"""GPU: true peak and gain (BatchDecoder.set_true_peak / true_peak /
decode_measure / normalize_gain / apply_gain / decode_normalized;
include/mp3d.h "true peak and gain").

Reference: the header's definition in float64 numpy with the float32 taps
(tests/test_normalize_host.py: truepeak64, gain64, int16_of).  Bound, from the
header: with P the largest |x| of the stream since its restart,
    |tpeak - ref| <= 23 * 2^-24 * P
(12 float32 roundings of a chain whose sum of |taps| is at most 1.856).  The
bound is derived, not measured; the value test prints max(err / bound) per
signal class (DESIGN.md section 4f records them).  Measured on an MI355X, the
largest of the four formats: unit impulse 0, fs/4 sine 0.097, noise 0.125, DC
0.134, one stream of 41 tiles 0.061.  Everything else here is exact: a maximum
has one value whatever the order, a gain is one float32 multiply, the int16
conversion is the packed sink's.
"""
import re

import numpy as np
import pytest
import torch

import mp3_amd
from mp3_amd import _build
from test_gpu_features import FS, Batch
from test_gpu_loudness import Tagged
from test_normalize_host import gain64, int16_of, truepeak64

pytestmark = pytest.mark.gpu

_hdr = (_build.CSRC / "mp3d_normalize.h").read_text()
TILE = int(re.search(r"^#define MP3D_TP_TILE\s+(\d+)", _hdr, re.M).group(1))
CHUNK = int(re.search(r"^#define MP3D_GA_CHUNK\s+(\d+)", _hdr, re.M).group(1))
FORMATS = [(48000, 2), (44100, 2), (11025, 1), (8000, 1)]
# the look-ahead of 6, the history of 11 and both sides of a tile edge
LENS = [0, 1, 5, 6, 7, 11, 12, 17, TILE - 1, TILE, TILE + 6, TILE + 7, 3 * TILE + 17]
NMAX = LENS[-1]
PATTERN = np.float32(-777.25)
BOUND = 23.0 * 2.0 ** -24


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- signals and reference -------------------------------------------------------
def signals(fs, ch, n):
    """{class: float32 [n, ch]}: the second channel differs from the first."""
    rng = np.random.default_rng(31770 + fs + ch)
    t = np.arange(n)
    imp = np.zeros((n, ch), np.float32)
    imp[0, 0] = 1.0
    # full scale at fs / 4, sampled at 45 degrees: every sample is +-0.7071, the peak between them is 1
    sine = np.stack([(1.0 - 0.25 * c) * np.sin(0.5 * np.pi * t + 0.25 * np.pi) for c in range(ch)], 1).astype(np.float32)
    noise = rng.uniform(-1.0, 1.0, (n, ch)).astype(np.float32)
    dc = np.full((n, ch), 0.9, np.float32)
    if ch == 2:
        imp[5, 1] = -1.0
        dc[:, 1] = -0.45
    return {"impulse": imp, "fs/4 sine": sine, "noise": noise, "dc": dc}


_sig, _ref = {}, {}


def sig(fs, ch, n=NMAX):
    if (fs, ch, n) not in _sig:
        _sig[(fs, ch, n)] = signals(fs, ch, n)
    return _sig[(fs, ch, n)]


def ref(x, key, k, flush):
    """truepeak64 of x[:k], flushed or not: computed once per key, never changed."""
    key = key + (k, flush)
    if key not in _ref:
        _ref[key] = truepeak64(x[:k], k if flush else max(k - 6, 0))
    return _ref[key]


def check(got, want, x, what):
    """One float32 true peak against the float64 one for the stream fed x; returns err / bound."""
    P = float(np.abs(x).max(initial=0.0))
    err = abs(float(got) - want)
    assert err <= BOUND * P, (what, float(got), want, err / (BOUND * P) if P else np.inf)
    return err / (BOUND * P) if P else 0.0


# ---- the tap ---------------------------------------------------------------------
def handle(n, fs, ch, F=1, loud=False):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(fs, ch)
    if loud:
        dec.set_loudness(True)
    dec.set_true_peak(True)
    return dec


def tap(dec, xs, flush=False):
    """Feed xs[s] ([k, ch]) to stream s in one call; returns tpeak float32 [n]."""
    n, ch = len(xs), dec._out[1]
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss, ch), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    tp = dec.true_peak(smp, np.array([len(x) for x in xs], np.int32), tpeak=np.full(n, PATTERN), flush=flush)
    assert tp.dtype == np.float32 and (tp >= 0.0).all()
    return tp


def run_tap_case(fs, ch):
    """{class: (tpeak of the LENS streams flushed, the same not flushed)} of one call each."""
    out = {}
    for name, x in sig(fs, ch).items():
        xs = [x[:k] for k in LENS]
        out[name] = (tap(handle(len(LENS), fs, ch), xs, flush=True), tap(handle(len(LENS), fs, ch), xs))
    return out


_tap = {}


def tap_case(fs, ch):
    if (fs, ch) not in _tap:
        _tap[(fs, ch)] = run_tap_case(fs, ch)
    return _tap[(fs, ch)]


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_tap_values(fs, ch):
    for name, (flushed, open_) in tap_case(fs, ch).items():
        x = sig(fs, ch)[name]
        worst = 0.0
        for s, k in enumerate(LENS):
            what = "%d Hz x %d, %s, %d samples" % (fs, ch, name, k)
            worst = max(worst, check(flushed[s], ref(x, (fs, ch, name), k, True), x[:k], what + ", flushed"))
            worst = max(worst, check(open_[s], ref(x, (fs, ch, name), k, False), x[:k], what))
            # phase 0 is the signal itself: never below the sample peak
            assert flushed[s] >= np.abs(x[:k]).max(initial=0.0), what
            if k <= 6:
                assert open_[s] == 0.0, what  # nothing is emitted before sample n + 6
            if name == "impulse":
                assert flushed[s] == (1.0 if k else 0.0), what
        print("tap %d Hz x %d, %s: max err/bound %.3g" % (fs, ch, name, worst))
    # the inter-sample peak is seen: samples of +-0.7071, a true peak above 1
    assert tap_case(fs, ch)["fs/4 sine"][0][-1] > 1.01


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_split_invariance(fs, ch):
    for name, x in sig(fs, ch).items():
        whole = tap_case(fs, ch)[name][0][-1]
        for sizes in ([1, 5, 6, 11, TILE, NMAX - TILE - 23], [1] * 40 + [NMAX - 40]):
            assert sum(sizes) == NMAX
            dec = handle(1, fs, ch)
            got, a = np.float32(0.0), 0
            for i, k in enumerate(sizes):
                tp = tap(dec, [x[a:a + k]], flush=i == len(sizes) - 1)[0]
                if a + k <= 6:
                    assert tp == 0.0
                got = max(got, tp)
                a += k
            assert same_bits(got, whole), (name, sizes[:6], float(got), float(whole))


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_flush_and_restarts(fs, ch):
    x = sig(fs, ch)["noise"]
    k = TILE + 9
    dec = handle(1, fs, ch)
    first = tap(dec, [x[:k]], flush=True)
    assert same_bits(tap(dec, [x[:k]], flush=True), first)  # the flush restarted the stream
    # a flush with nothing new emits the six indices held back
    dec = handle(1, fs, ch)
    held = tap(dec, [x[:k]])
    rest = tap(dec, [x[:0]], flush=True)
    assert same_bits(np.maximum(held, rest), first)

    # a loud sample at the end of a call is not emitted by it: it waits in the history
    loud = 0.01 * x[:20].copy()
    loud[19] = 4.0
    quiet = 0.01 * x[20:300]
    fresh = tap(handle(1, fs, ch), [quiet], flush=True)
    cont = handle(1, fs, ch)
    assert tap(cont, [loud])[0] < 0.05
    goes_on = tap(cont, [quiet], flush=True)
    assert goes_on[0] >= 4.0 and fresh[0] < 0.05

    def second_call(restart):
        dec = handle(3, fs, ch)
        tap(dec, [loud] * 3)
        restart(dec)
        return tap(dec, [quiet] * 3, flush=True)

    blob = mp3_amd.BatchDecoder(1, 1).get_state(0, 1)
    for what, restart, slots in [("reset", lambda d: d.reset(), (0, 1, 2)),
                                 ("set_state", lambda d: d.set_state(blob, first=1), (1,)),
                                 ("set_window", lambda d: d.set_window([0], first=1), (1,)),
                                 ("set_true_peak", lambda d: d.set_true_peak(True), (0, 1, 2))]:
        got = second_call(restart)
        for s in range(3):
            assert same_bits(got[s], fresh[0] if s in slots else goes_on[0]), (what, s)
    dec = handle(1, fs, ch)
    tap(dec, [loud])
    dec.set_output(fs, ch)  # any set_output turns the tap off
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.true_peak(loud[None], [20])
    dec.set_true_peak(True)
    assert same_bits(tap(dec, [quiet], flush=True), fresh)
    dec.set_true_peak(False)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.true_peak(loud[None], [20])


def test_one_long_stream():
    fs, n = 48000, 40 * TILE + 3
    x = (np.random.default_rng(78).uniform(-0.6, 0.6, (n, 1)) + 0.3).astype(np.float32)
    got = tap(handle(3, fs, 1), [x], flush=True)
    print("one long stream, %d tiles: err/bound %.3g" % (-(-n // TILE), check(got[0], truepeak64(x, n), x, "long")))
    assert same_bits(tap(handle(1, fs, 1), [x], flush=True), got)


# ---- decode_measure --------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    return Tagged(Batch())


def packed_on_device(dec, batch, gapless=False):
    """decode_packed(flush) into device tensors: (out, counts)."""
    fs, ch = dec._out
    offs, sizes = batch.geom(0, FS)
    S = mp3_amd.packed_max_samples(fs, FS)
    out = torch.zeros((batch.n, S, ch), dtype=torch.float32, device="cuda")
    counts = torch.zeros((batch.n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_packed(batch.blob, offs, sizes, FS, out=out, counts=counts, flush=True, gapless=gapless)
    dec.sync()
    return out, counts


@pytest.mark.parametrize("gapless", [False, True])
@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_decode_measure(batch, fs, ch, gapless):
    offs, sizes = batch.geom(0, FS)
    stride = mp3_amd.loud_max_blocks(fs, FS)
    blocks, bc, pk, tp, _ = handle(batch.n, fs, ch, F=FS, loud=True).decode_measure(
        batch.blob, offs, sizes, FS, blocks=np.full((batch.n, stride), PATTERN), tpeak=np.full(batch.n, PATTERN),
        flush=True, gapless=gapless)
    twin = mp3_amd.BatchDecoder(batch.n, FS)
    twin.set_output(fs, ch)
    twin.set_loudness(True)
    wb, wc, wpk, _ = twin.decode_loudness(batch.blob, offs, sizes, FS, blocks=np.full((batch.n, stride), PATTERN),
                                          flush=True, gapless=gapless)
    assert np.array_equal(bc, wc) and same_bits(blocks, wb) and same_bits(pk, wpk)
    assert bc.max() >= 3
    dec = handle(batch.n, fs, ch, F=FS)
    out, counts = packed_on_device(dec, batch, gapless)
    want = dec.true_peak(out, counts, flush=True)
    assert same_bits(tp, want)
    smp, cnt = out.cpu().numpy(), counts.cpu().numpy()
    for s in range(batch.n):
        x = smp[s, : cnt[s]]
        check(tp[s], truepeak64(x, len(x)), x, batch.names[s])
        assert tp[s] >= pk[s]
    assert tp[batch.names.index("empty")] == 0.0 and tp.max() > 0.0


def test_decode_measure_in_calls(batch):
    """Frame slots in two calls: the max over the calls is the one-call value."""
    fs, ch = 48000, 2
    dec = handle(batch.n, fs, ch, F=FS, loud=True)
    got = np.zeros(batch.n, np.float32)
    for a, b, last in [(0, 5, False), (5, FS, True)]:
        offs, sizes = batch.geom(a, b)
        got = np.maximum(got, dec.decode_measure(batch.blob, offs, sizes, b - a, flush=last)[3])
    offs, sizes = batch.geom(0, FS)
    whole = handle(batch.n, fs, ch, F=FS, loud=True).decode_measure(batch.blob, offs, sizes, FS, flush=True)[3]
    assert same_bits(got, whole)


# ---- the gain rule ---------------------------------------------------------------
def test_normalize_gain():
    lufs = np.array([-np.inf, np.nan, -70.0, -23.0, -5.0], np.float32)
    tps = np.array([0.0, 0.25, 1.0, 1.7], np.float32)
    L, T = (a.reshape(-1).copy() for a in np.meshgrid(lufs, tps, indexing="ij"))
    n = L.size
    dec = mp3_amd.BatchDecoder(n, 1)
    acted = 0
    for target in (-23.0, -14.0):
        for max_dbtp in (-1.0, 0.0):
            c = 10.0 ** (max_dbtp / 20.0)
            g = dec.normalize_gain(L, T, target=target, max_dbtp=max_dbtp, gain=np.full(n, PATTERN))
            free = dec.normalize_gain(L, None, target=target, max_dbtp=max_dbtp)
            for s in range(n):
                want, unl = gain64(L[s], T[s], target, max_dbtp), gain64(L[s], None, target, max_dbtp)
                assert abs(float(g[s]) - float(want)) <= 2.0 ** -23 * float(want), (s, g[s], want)
                assert abs(float(free[s]) - float(unl)) <= 2.0 ** -23 * float(unl), (s, free[s], unl)
                if not np.isfinite(L[s]):
                    assert g[s] == 1.0 and free[s] == 1.0  # exactly, whatever the peak
                elif want != unl:  # the limit acts
                    acted += 1
                    assert float(g[s]) * float(T[s]) <= c * (1.0 + 2.0 ** -22), (s, g[s])
            dl, dt = torch.from_numpy(L).cuda(), torch.from_numpy(T).cuda()
            dg = torch.full((n,), float(PATTERN), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dec.normalize_gain(dl, dt, target=target, max_dbtp=max_dbtp, gain=dg)
            dec.sync()
            assert same_bits(dg.cpu().numpy(), g)
    assert acted >= 8
    short = dec.normalize_gain(L[:3], T[:3], gain=np.full(5, PATTERN))
    assert (short[3:] == PATTERN).all()  # nothing past n_streams


# ---- apply -----------------------------------------------------------------------
S_APPLY = 9002  # rows of both paths: some 16-byte aligned, some not; more than one chunk
GAINS = np.array([0.5, 1.7, 0.25, 1.0, 3.0, 0.8], np.float32)


def apply_input(ch):
    rng = np.random.default_rng(555 + ch)
    x = rng.uniform(-1.2, 1.2, (len(GAINS), S_APPLY, ch)).astype(np.float32)
    # stream 0 (gain 0.5, exact): products on the .5 ties of the int16 conversion, and beyond full scale
    k = np.array([0, 1, 2, -1, -2, -3, 12345, -12345, 32766, 32767, -32768, -32769, 40000, -40000], np.float64)
    x[0, 100:100 + k.size, 0] = ((2.0 * k + 1.0) / 32768.0).astype(np.float32)
    x[0, 200:204, ch - 1] = [2.5, -2.5, 1.0, -1.0]
    counts = np.array([S_APPLY, CHUNK // ch + 1, 0, -1, 5, S_APPLY + 7], np.int32)
    assert S_APPLY * ch > CHUNK
    return x, counts


def run_apply_case(ch):
    """The outputs of apply_gain on pattern-filled buffers: float32 and int16, device and host, and in place."""
    x, counts = apply_input(ch)
    dec = mp3_amd.BatchDecoder(len(GAINS), 1)
    dec.set_output(48000, ch)
    dx, dc, dg = torch.from_numpy(x).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(GAINS).cuda()
    d32 = torch.full(x.shape, float(PATTERN), dtype=torch.float32, device="cuda")
    d16 = torch.full(x.shape, -77, dtype=torch.int16, device="cuda")
    inplace = dx.clone()
    torch.cuda.synchronize()
    dec.apply_gain(dx, dc, dg, out=d32)
    dec.apply_gain(dx, dc, dg, out=d16, f32=False)
    dec.apply_gain(inplace, dc, dg, out=inplace)
    dec.sync()
    h32 = dec.apply_gain(x, counts, GAINS, out=np.full(x.shape, PATTERN, np.float32))
    h16 = dec.apply_gain(x, counts, GAINS, out=np.full(x.shape, -77, np.int16), f32=False)
    mixed = dec.apply_gain(dx, counts, dg, out=np.full(x.shape, PATTERN, np.float32))  # device in, host out
    return {"d32": d32.cpu().numpy(), "d16": d16.cpu().numpy(), "inplace": inplace.cpu().numpy(), "h32": h32,
            "h16": h16, "mixed": mixed}


_apply = {}


def apply_case(ch):
    if ch not in _apply:
        _apply[ch] = run_apply_case(ch)
    return _apply[ch]


@pytest.mark.parametrize("ch", [2, 1])
def test_apply_gain(ch):
    x, counts = apply_input(ch)
    got = apply_case(ch)
    want32 = np.full(x.shape, PATTERN, np.float32)
    want16 = np.full(x.shape, -77, np.int16)
    keep = x.copy()
    for s, c in enumerate(np.clip(counts, 0, S_APPLY)):
        y = x[s, :c] * GAINS[s]  # one float32 multiply
        assert y.dtype == np.float32
        want32[s, :c], keep[s, :c], want16[s, :c] = y, y, int16_of(y)
    assert same_bits(got["d32"], want32)  # bit for bit, and nothing past the counts
    assert np.array_equal(got["d16"], want16)
    assert same_bits(got["inplace"], keep)
    assert same_bits(got["h32"], want32) and same_bits(got["mixed"], want32) and np.array_equal(got["h16"], want16)
    ties = want16[0, 100:114, 0]
    assert list(ties) == [1, 2, 3, 0, -1, -2, 12346, -12344, 32767, 32767, -32767, -32768, 32767, -32768]
    assert want32[0, 200, ch - 1] == 1.25 and want32[0, 201, ch - 1] == -1.25  # float32 is not clipped


# ---- buffers, errors, timing -----------------------------------------------------
@pytest.mark.parametrize("fs,ch", [(48000, 2), (8000, 1)])
def test_host_and_device_buffers_agree(fs, ch):
    want = tap_case(fs, ch)["noise"]
    x = sig(fs, ch)["noise"]
    smp = torch.zeros((len(LENS), NMAX, ch), dtype=torch.float32, device="cuda")
    for s, k in enumerate(LENS):
        smp[s, :k] = torch.from_numpy(x[:k]).cuda()
    strm = torch.cuda.Stream()
    for flush in (True, False):
        with torch.cuda.stream(strm):
            cnt = torch.tensor(LENS, dtype=torch.int32, device="cuda")
            tp = torch.full((len(LENS),), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dec = handle(len(LENS), fs, ch)
            dec.true_peak(smp, cnt, tpeak=tp, flush=flush, stream=strm.cuda_stream)
        strm.synchronize()
        assert same_bits(tp.cpu().numpy(), want[0 if flush else 1])


def test_argument_errors(batch):
    fs, ch = 48000, 2
    L = mp3_amd.lib()
    x = np.ascontiguousarray(sig(fs, ch)["noise"][None, :5000])
    dec = mp3_amd.BatchDecoder(2, 1)
    assert L.mp3d_batch_set_true_peak(dec._h, 1) == -1  # no packed format yet
    cnt, tp, g = np.array([5000, 0], np.int32), np.zeros(2, np.float32), np.ones(2, np.float32)
    out = np.zeros((2, 5000, ch), np.float32)

    def apply(n=1, sp=x.ctypes.data, op=out.ctypes.data, f32=1, gp=g.ctypes.data, stride=5000):
        return L.mp3d_batch_apply_gain(dec._h, sp, stride, cnt.ctypes.data, n, gp, op, f32, None)

    assert apply() == -1  # apply_gain needs the format's channel count
    dec.set_output(fs, ch)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.true_peak(x, [5000])  # before set_true_peak
    offs, sizes = batch.geom(0, 1)
    for loud, tpk in [(True, False), (False, True)]:  # decode_measure needs both sinks
        dec.set_loudness(loud)
        dec.set_true_peak(tpk)
        with pytest.raises(mp3_amd.MP3DError, match="-1"):
            dec.decode_measure(batch.blob, offs[:2], sizes[:2], 1)
    with pytest.raises(mp3_amd.MP3DError):
        dec.decode_normalized(batch.blob, offs[:2], sizes[:2], 1)
    dec.set_loudness(True)

    def call(flags, n=1, sp=x.ctypes.data, tpp=tp.ctypes.data, stride=5000, cp=cnt.ctypes.data):
        return L.mp3d_batch_true_peak(dec._h, sp, stride, cp, n, tpp, flags, None)

    assert call(4) == -1  # an unknown flag
    assert call(mp3_amd.PACK_GAPLESS) == -1  # the tap has no frames to read a tag from
    assert call(0, n=3) == -5  # more streams than the handle has
    assert call(0, n=0) == -1
    assert call(0, tpp=None) == -1 and call(0, cp=None) == -1 and call(0, sp=None) == -1
    assert call(0, stride=-1) == -1
    dsmp = torch.zeros(2 * 5000 * ch + 4, dtype=torch.float32, device="cuda")
    dtp = torch.zeros(8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert call(0, sp=dsmp.data_ptr() + 2) == -1  # a misaligned device pointer
    assert call(0, tpp=dtp.data_ptr() + 1) == -1
    assert call(0) == 0 and tp[0] >= np.abs(x[0, :4994]).max()
    assert call(mp3_amd.PACK_FLUSH, sp=dsmp.data_ptr() + 4, tpp=dtp.data_ptr() + 4) == 0
    # device pointers must be int-aligned: counts as well
    dcnt = torch.tensor([0, 5000, 0, 0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert call(0, cp=dcnt.data_ptr() + 1) == -1 and call(0, cp=dcnt.data_ptr() + 2) == -1
    assert call(mp3_amd.PACK_FLUSH) == 0
    want, tp[0] = tp[0], 0.0
    assert want > 0.0 and call(mp3_amd.PACK_FLUSH, cp=dcnt.data_ptr() + 4) == 0 and tp[0] == want
    blocks, bc = np.zeros((2, 4), np.float32), np.zeros(2, np.int32)

    def measure(flags, tpp=tp.ctypes.data, n=2, F=1):
        return L.mp3d_batch_decode_measure(dec._h, batch.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, n, F,
                                           blocks.ctypes.data, 4, bc.ctypes.data, None, tpp, flags, None, None)

    assert measure(4) == -1 and measure(0, tpp=None) == -1 and measure(0, n=3) == -5 and measure(0, F=2) == -5
    assert measure(mp3_amd.PACK_FLUSH | mp3_amd.PACK_GAPLESS) == 0

    def gain(n=2, lp=tp.ctypes.data, gp=g.ctypes.data, target=-23.0):
        return L.mp3d_batch_normalize_gain(dec._h, lp, None, n, target, -1.0, gp, None)

    assert gain(lp=None) == -1 and gain(gp=None) == -1 and gain(n=0) == -1 and gain(n=3) == -5
    assert gain(target=float("nan")) == -1 and gain(lp=dtp.data_ptr() + 1) == -1
    assert gain() == 0

    assert apply(op=None) == -1 and apply(gp=None) == -1 and apply(n=0) == -1 and apply(n=3) == -5
    assert apply(stride=-1) == -1 and apply(sp=None) == -1
    assert apply(op=x.ctypes.data, f32=0) == -1  # in place is for float32
    dout = torch.zeros(2 * 5000 * ch + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert apply(op=dout.data_ptr() + 4) == -1  # a device out is aligned to one sample frame
    assert apply(op=dout.data_ptr() + 2, f32=0) == -1
    assert apply(sp=dsmp.data_ptr() + 2) == -1
    assert apply(op=dout.data_ptr() + 8) == 0 and apply(op=dout.data_ptr() + 4, f32=0) == 0 and apply() == 0
    dec.sync()


def test_true_peak_time(batch):
    dec = handle(batch.n, 48000, 2, F=FS, loud=True)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.true_peak_time_us()  # no true-peak call yet
    offs, sizes = batch.geom(0, FS)
    dec.decode_measure(batch.blob, offs, sizes, FS, flush=True)
    assert dec.true_peak_time_us() > 0.0 and dec.loudness_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- the whole-file call ---------------------------------------------------------
@pytest.mark.parametrize("fs,ch,target", [(48000, 2, -16.0), (11025, 1, -23.0)])
def test_decode_normalized(batch, fs, ch, target):
    max_dbtp = -1.0
    c = 10.0 ** (max_dbtp / 20.0)
    F = batch.F  # the streams whole: the longer ones pass 400 ms and have a loudness, the 16-frame ones have none
    offs, sizes = batch.geom()
    out, counts, lufs, tp, gain, infos = handle(batch.n, fs, ch, F=F, loud=True).decode_normalized(
        batch.blob, offs, sizes, F, target=target, max_dbtp=max_dbtp)
    # the composition, call by call
    dec = handle(batch.n, fs, ch, F=F, loud=True)
    smp, cnt, winfos = dec.decode_packed(batch.blob, offs, sizes, F, flush=True)
    blocks, bc, _ = dec.loudness(smp, cnt, flush=True)
    wtp = dec.true_peak(smp, cnt, flush=True)
    wl = dec.integrated_lufs(blocks, bc)
    wg = dec.normalize_gain(wl, wtp, target=target, max_dbtp=max_dbtp)
    want = dec.apply_gain(smp, cnt, wg)
    assert np.array_equal(counts, cnt) and np.array_equal(infos, winfos)
    assert same_bits(lufs, wl) and same_bits(tp, wtp) and same_bits(gain, wg) and same_bits(out, want)
    out16 = handle(batch.n, fs, ch, F=F, loud=True).decode_normalized(batch.blob, offs, sizes, F, target=target,
                                                                       max_dbtp=max_dbtp, f32=False)[0]
    assert out16.dtype == np.int16 and np.array_equal(out16, int16_of(out))
    # Measured again, the output is at the target and under the ceiling.  The 1e-4 LU: the gain and every scaled
    # sample are float32 (2^-24 each: 1e-6 dB together), and the loudness before and after is stored as float32,
    # whose ulp is 1.9e-6 at 16 .. 32 LU and 3.8e-6 above; 1e-4 is 25 such steps.  Measured on an MI355X: 1.9e-6.
    blocks, bc, _ = dec.loudness(out, counts, flush=True)
    after = dec.integrated_lufs(blocks, bc)
    tp_after = dec.true_peak(out, counts, flush=True)
    free, worst = 0, 0.0
    for s in range(batch.n):
        if not np.isfinite(lufs[s]):  # no loudness, no gain: the rule leaves the stream as it is, limit included
            assert gain[s] == 1.0 and same_bits(out[s], smp[s]) and same_bits(tp_after[s], tp[s])
            continue
        assert tp_after[s] <= c * (1.0 + 2.0 ** -20), (batch.names[s], tp_after[s])
        if gain[s] == gain64(lufs[s], None, target, max_dbtp):  # the limit did not act
            free += 1
            worst = max(worst, abs(float(after[s]) - target))
            assert abs(float(after[s]) - target) <= 1e-4, (batch.names[s], after[s])
    print("decode_normalized %d Hz x %d to %g LUFS: %d of %d streams free of the limit, max |lufs - target| %.2g LU"
          % (fs, ch, target, free, batch.n, worst))
    assert free >= 1 and (gain == 1.0).any() and (gain != 1.0).any()


# ---- poison ----------------------------------------------------------------------
def assert_same_cases(fs, ch):
    for name, (flushed, open_) in run_tap_case(fs, ch).items():
        want = tap_case(fs, ch)[name]
        assert same_bits(flushed, want[0]) and same_bits(open_, want[1]), name
    got, want = run_apply_case(ch), apply_case(ch)
    for key in want:
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_poison(fs, ch, monkeypatch):
    tap_case(fs, ch), apply_case(ch)  # (the product library's, without the poison)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    assert_same_cases(fs, ch)


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_workgroup_lds_poison_build(fs, ch, monkeypatch):
    tap_case(fs, ch), apply_case(ch)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        assert_same_cases(fs, ch)
