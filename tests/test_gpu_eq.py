"""The equaliser sink on the GPU (include/mp3d.h "equaliser sink"; DESIGN.md
section 4j) against the float64 sequential reference of tests/_eq.py:

    |y - ref| <= 2^-22 |ref| + EPS G,  G the running peak of |ref|

over the formats, curves, signals and lengths of tests/_eq.py as ragged
streams of one batch; split invariance; one stream past the 64 tiles of a
carry scan; decode_equalized against eq on decode_packed's samples; restarts,
the other sinks' state, argument errors, host and device buffers, the debug
builds and the stage timer.  EPS comes from the CPU measurement of
tests/test_eq_host.py, never from what the GPU returns."""
import numpy as np
import pytest
import torch

import _eq
import mp3_amd
from mp3_amd import _build
from test_gpu_features import FS, Batch

pytestmark = pytest.mark.gpu

SEG, TILE = _eq.SEG, _eq.TILE
PATTERN = np.float32(-777.25)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def handle(n, fs, ch, curve, F=1):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(fs, ch)
    dec.set_eq(*_eq.curve(curve, fs))
    return dec


def feed(dec, xs, flush=False, stride=None):
    """Feed xs[s] ([k, ch]) to stream s in one call: ([out of s], counts, raw out)."""
    n, (fs, ch) = len(xs), dec._out
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss, ch), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    cnt = np.array([len(x) for x in xs], np.int32)
    out = np.full((n, ss + 3 if stride is None else stride, ch), PATTERN, np.float32)
    out, oc = dec.eq(smp, cnt, out=out, flush=flush)
    for s in range(n):
        assert (out[s, max(int(oc[s]), 0):] == PATTERN).all(), s  # nothing past the count is touched
    return [out[s, : max(int(oc[s]), 0)].copy() for s in range(n)], oc, out


# ---- values ------------------------------------------------------------------------------
_val = {}


def run_values(fs, ch, curve):
    xs = [x for _, _, x in _eq.streams(fs, ch)]
    got, oc, _ = feed(handle(len(xs), fs, ch, curve), xs)
    assert list(oc) == [len(x) for x in xs]
    return got


def values(fs, ch, curve):
    if (fs, ch, curve) not in _val:
        _val[(fs, ch, curve)] = run_values(fs, ch, curve)
    return _val[(fs, ch, curve)]


@pytest.mark.parametrize("curve", _eq.CURVES)
@pytest.mark.parametrize("fs,ch", _eq.FORMATS)
def test_values(fs, ch, curve):
    got = values(fs, ch, curve)
    worst = (0.0, None)
    for (name, n, x), y, (_, r) in zip(_eq.streams(fs, ch), got, _eq.reference(fs, ch, curve)):
        assert y.shape == (n, ch)
        e = _eq.excess(y, r)
        worst = max(worst, (e, (name, n)), key=lambda t: t[0])
        if curve == "flat":  # an identity that needs no oracle
            assert _eq.excess(y, x.astype(np.float64)) <= 1.0, (name, n)
    print("%d Hz x %d, %s: max err/bound %.3g at %s" % (fs, ch, curve, worst[0], worst[1]))
    assert worst[0] <= 1.0, worst


# ---- split invariance ------------------------------------------------------------------------
def in_pieces(fs, ch, curve, xs, sizes):
    """the streams fed in calls of the given sizes in turn (the last one whatever is left)"""
    dec = handle(len(xs), fs, ch, curve)
    n = max(len(x) for x in xs)
    got, a, i = [[] for _ in xs], 0, 0
    while a < n:
        p = sizes[i % len(sizes)]
        out, oc, _ = feed(dec, [x[a:a + p] for x in xs])
        assert list(oc) == [len(x[a:a + p]) for x in xs]
        for s, o in enumerate(out):
            got[s].append(o)
        a, i = a + p, i + 1
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize("fs,ch,curve", [(48000, 2, "pole20"), (48000, 2, "graphic"), (8000, 1, "graphic")])
def test_split_invariance(fs, ch, curve):
    long = max(_eq.LENGTHS)
    pick = [s for s, (_, n, _) in enumerate(_eq.streams(fs, ch)) if n == long]
    xs = [_eq.streams(fs, ch)[s][2] for s in pick]
    refs = [_eq.reference(fs, ch, curve)[s][1] for s in pick]
    one = [values(fs, ch, curve)[s] for s in pick]
    short = 5 * SEG + 3
    worst = 0.0
    for what, sizes, k in [("1, 7, SEG, TILE, TILE + 1 in turn", (1, 7, SEG, TILE, TILE + 1), long),
                           ("TILE", (TILE,), long), ("TILE + 1", (TILE + 1,), long),
                           ("1", (1,), short), ("7", (7,), short), ("SEG", (SEG,), short)]:
        got = in_pieces(fs, ch, curve, [x[:k] for x in xs], sizes)
        for y, y1, r in zip(got, one, refs):
            assert _eq.excess(y, r[:k]) <= 1.0, what
            b = _eq.bound(r[:k])
            d = np.abs(y.astype(np.float64) - y1[:k].astype(np.float64))
            assert (d <= b).all(), what
            worst = max(worst, float((d[b > 0] / b[b > 0]).max(initial=0.0)))
    print("%d Hz x %d, %s: largest split difference / bound %.3g" % (fs, ch, curve, worst))


# ---- one long stream ---------------------------------------------------------------------------
LONG_N = 66 * TILE + 1234  # past the 64 tiles of one carry scan
_long = {}


def long_case():
    """noise through curve 1 at 48 kHz stereo and curve 2 at 8 kHz mono: (x, coef) per case and
    the references, from one run of the sample loop (the shorter cascade padded with exact
    identity stages)"""
    if not _long:
        cases = [(48000, 2, "pole20"), (8000, 1, "graphic")]
        xs = [_eq.signal("noise", fs, LONG_N, ch, seed=66) for fs, ch, _ in cases]
        coefs = [_eq.design64(fs, *_eq.curve(c, fs)) for fs, _, c in cases]
        K = max(len(c) for c in coefs)
        lane_coef = []
        for c, x in zip(coefs, xs):
            pad = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 0.0]), (K - len(c), 1))
            lane_coef += [np.concatenate([c, pad])] * x.shape[1]
        y = _eq.seq(np.stack(lane_coef, -1), np.concatenate(xs, 1))
        a = 0
        for (fs, ch, c), x in zip(cases, xs):
            _long[(fs, ch, c)] = (x, y[:, a:a + ch].copy())
            a += ch
    return _long


@pytest.mark.parametrize("fs,ch,curve", [(48000, 2, "pole20"), (8000, 1, "graphic")])
def test_one_long_stream(fs, ch, curve):
    x, r = long_case()[(fs, ch, curve)]
    got, oc, _ = feed(handle(1, fs, ch, curve), [x])
    assert list(oc) == [LONG_N]
    e = _eq.excess(got[0], r)
    print("one stream of %d tiles, %d Hz x %d, %s: max err/bound %.3g" % (-(-LONG_N // TILE), fs, ch, curve, e))
    assert e <= 1.0


# ---- decode_equalized against the stage on the packed samples ----------------------------------
@pytest.fixture(scope="module")
def batch():
    return Batch()


DEC_FMT = (48000, 2)


def packed_on_device(batch, dec, gapless, frames=(0, FS), flush=True):
    fs, ch = dec._out
    a, b = frames
    offs, sizes = batch.geom(a, b)
    S = mp3_amd.packed_max_samples(fs, b - a)
    out = torch.zeros((batch.n, S, ch), dtype=torch.float32, device="cuda")
    counts = torch.zeros((batch.n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_packed(batch.blob, offs, sizes, b - a, out=out, counts=counts, flush=flush, gapless=gapless)
    dec.sync()
    return out, counts


@pytest.mark.parametrize("gapless", [False, True])
def test_decode_equalized_is_the_stage_on_the_packed_samples(batch, gapless):
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, "graphic", F=FS)
    smp, counts = packed_on_device(batch, dec, gapless)
    S = smp.shape[1]
    via, vc = dec.eq(smp, counts, flush=True, stride=S)
    dec.sync()
    offs, sizes = batch.geom(0, FS)
    comp = handle(batch.n, fs, ch, "graphic", F=FS)
    out = np.full((batch.n, S, ch), PATTERN, np.float32)
    out, oc, _ = comp.decode_equalized(batch.blob, offs, sizes, FS, out=out, flush=True, gapless=gapless)
    cnt = counts.cpu().numpy()
    assert np.array_equal(oc, cnt) and np.array_equal(vc, cnt)
    assert oc[batch.names.index("empty")] == 0 and oc.max() > TILE
    x = smp.cpu().numpy()
    ref_coef = _eq.design64(fs, *_eq.curve("graphic", fs))
    for s in range(batch.n):
        assert same_bits(out[s, : oc[s]], via[s, : oc[s]]), batch.names[s]
        assert (out[s, oc[s]:] == PATTERN).all(), batch.names[s]
    for s in (0, 2):  # and the definition itself, on decoded audio
        assert _eq.excess(out[s, : oc[s]], _eq.seq(ref_coef, x[s, : oc[s]])) <= 1.0


def test_decode_equalized_leaves_decoder_and_resampler_as_decode_packed_does(batch):
    fs, ch = DEC_FMT
    a = handle(batch.n, fs, ch, "five_types", F=FS)
    b = mp3_amd.BatchDecoder(batch.n, FS)
    b.set_output(fs, ch)
    offs, sizes = batch.geom(0, 5)
    a.decode_equalized(batch.blob, offs, sizes, 5)
    b.decode_packed(batch.blob, offs, sizes, 5)
    assert np.array_equal(a.get_state(), b.get_state())
    assert all(np.array_equal(p, q) for p, q in zip(a.sink_window(), b.sink_window()))
    offs, sizes = batch.geom(5, FS)
    pa, ca, _ = a.decode_packed(batch.blob, offs, sizes, FS - 5, flush=True)
    pb, cb, _ = b.decode_packed(batch.blob, offs, sizes, FS - 5, flush=True)
    assert np.array_equal(ca, cb) and same_bits(pa, pb)  # the resamplers' tails included


# ---- lifecycle --------------------------------------------------------------------------------
def test_restarts_and_stride_overflow():
    fs, ch, curve = 48000, 2, "pole20"
    x = _eq.signal("noise", fs, TILE + 900, ch, seed=3)
    a, b = 700, TILE + 900
    cont = handle(1, fs, ch, curve)
    feed(cont, [x[:a]])
    goes_on = feed(cont, [x[a:b]])[0][0]
    fresh = feed(handle(1, fs, ch, curve), [x[a:b]])[0][0]
    assert not same_bits(goes_on, fresh)

    def second_call(restart):
        dec = handle(3, fs, ch, curve)
        feed(dec, [x[:a]] * 3)
        restart(dec)
        return feed(dec, [x[a:b]] * 3)[0]

    blob = mp3_amd.BatchDecoder(1, 1).get_state(0, 1)
    for what, restart, slots in [("reset", lambda d: d.reset(), (0, 1, 2)),
                                 ("set_state", lambda d: d.set_state(blob, first=1), (1,)),
                                 ("set_window", lambda d: d.set_window([0], first=1), (1,)),
                                 ("set_eq", lambda d: d.set_eq(*_eq.curve(curve, fs)), (0, 1, 2)),
                                 ("flush", lambda d: feed(d, [x[:0], x[:5], x[:0]], flush=True), (0, 1, 2))]:
        got = second_call(restart)
        for s in range(3):
            assert same_bits(got[s], fresh if s in slots else goes_on), (what, s)
    # a flush restarts after the call's samples
    dec = handle(1, fs, ch, curve)
    both = feed(dec, [x[:a]], flush=True)[0][0]
    assert same_bits(both, feed(handle(1, fs, ch, curve), [x[:a]])[0][0])
    assert same_bits(feed(dec, [x[a:b]])[0][0], fresh)
    # stride overflow: -1, nothing written, the slot restarted; the others go on
    dec = handle(3, fs, ch, curve)
    feed(dec, [x[:a]] * 3)
    got, oc, raw = feed(dec, [x[a:a + 20], x[a:a + 10], x[a:a + 11]], stride=10)
    assert list(oc) == [-1, 10, -1] and (raw[0] == PATTERN).all() and (raw[2] == PATTERN).all()
    cont = handle(1, fs, ch, curve)
    feed(cont, [x[:a]])
    assert same_bits(got[1], feed(cont, [x[a:a + 10]])[0][0])
    nxt = feed(dec, [x[a:b], x[a + 10:b], x[a:b]])[0]
    assert same_bits(nxt[0], fresh) and same_bits(nxt[2], fresh)
    # set_output turns the equaliser off, whatever the format; off and on again is a restart
    dec = handle(1, fs, ch, curve)
    feed(dec, [x[:a]])
    dec.set_output(fs, ch)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.eq(x[None, :a], [a])
    dec.set_eq(*_eq.curve(curve, fs))
    assert same_bits(feed(dec, [x[a:b]])[0][0], fresh)
    dec.set_eq(None)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.eq(x[None, :a], [a])
    # a rejected curve changes nothing
    dec = handle(1, fs, ch, curve)
    feed(dec, [x[:a]])
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.set_eq([(_eq.PEAK, 10.0, 0.0, 1.0)])
    assert same_bits(feed(dec, [x[a:b]])[0][0], goes_on)


def all_sinks(fs, ch, eq):
    dec = mp3_amd.BatchDecoder(1, 1)
    dec.set_output(fs, ch)
    dec.set_loudness(True)
    dec.set_true_peak(True)
    dec.set_stretch(True)
    dec.set_limiter(True, -1.0)
    dec.set_segments(True)
    if eq:
        dec.set_eq(*_eq.curve("graphic", fs))
    return dec


def others(dec, x):
    """every other sink fed x: all they return, as bytes"""
    smp, cnt = np.ascontiguousarray(x[None]), [len(x)]
    got = []
    for r in (dec.loudness(smp, cnt), dec.true_peak(smp, cnt), dec.stretch(smp, cnt), dec.limit(smp, cnt),
              dec.segments(smp, cnt)):
        got += [np.asarray(a).tobytes() for a in (r if isinstance(r, tuple) else (r,))]
    return got


def test_the_other_sinks_state_is_untouched():
    fs, ch = 44100, 2
    x = _eq.signal("noise", fs, 2 * TILE + 100, ch, seed=5) * np.float32(0.9)
    xa, xb = x[:TILE + 37], x[TILE + 37:]
    with_eq, without = all_sinks(fs, ch, True), all_sinks(fs, ch, False)
    a1 = others(with_eq, xa)
    e1 = feed(with_eq, [xa])[0][0]
    b1 = others(with_eq, xb)
    e2 = feed(with_eq, [xb])[0][0]
    assert a1 == others(without, xa) and b1 == others(without, xb)
    # ... and theirs leave the equaliser's alone
    only = handle(1, fs, ch, "graphic")
    assert same_bits(e1, feed(only, [xa])[0][0]) and same_bits(e2, feed(only, [xb])[0][0])


def test_argument_errors(batch):
    fs, ch = 48000, 2
    L = mp3_amd.lib()
    x = _eq.signal("noise", fs, 5000, ch)
    dec = mp3_amd.BatchDecoder(2, 1)
    bands = mp3_amd._eq_bands(_eq.curve("flat", fs)[0])
    assert L.mp3d_batch_set_eq(dec._h, bands.ctypes.data, bands.size, 0.0) == -1  # no packed format yet
    assert L.mp3d_batch_set_eq(dec._h, None, 0, 0.0) == 0  # off is always possible
    dec.set_output(fs, ch)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.eq(x[None], [5000])  # before set_eq
    offs, sizes = batch.geom(0, 1)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_equalized(batch.blob, offs[:2], sizes[:2], 1)
    assert L.mp3d_batch_set_eq(dec._h, bands.ctypes.data, -1, 0.0) == -1
    assert L.mp3d_batch_set_eq(dec._h, None, 3, 0.0) == -1
    assert L.mp3d_batch_set_eq(dec._h, bands.ctypes.data, bands.size, 24.5) == -1
    dec.set_eq(*_eq.curve("flat", fs))
    smp = np.ascontiguousarray(x[None])
    cnt, oc = np.array([5000], np.int32), np.zeros(1, np.int32)
    out = np.zeros((1, 5000, ch), np.float32)

    def call(flags=0, n=1, sp=smp.ctypes.data, op=out.ctypes.data, cp=cnt.ctypes.data, ocp=oc.ctypes.data, ss=5000,
             os=5000):
        return L.mp3d_batch_eq(dec._h, sp, ss, cp, n, op, os, ocp, flags, None)

    assert call(4) == -1  # an unknown flag
    assert call(mp3_amd.PACK_GAPLESS) == -1  # the stage has no frames to read a tag from
    assert call(n=3) == -5 and call(n=0) == -1  # more streams than the handle has
    assert call(ss=-1) == -1 and call(os=-1) == -1 and call(ss=2 ** 31) == -1 and call(os=2 ** 31) == -1
    assert call(op=None) == -1 and call(cp=None) == -1 and call(ocp=None) == -1 and call(sp=None) == -1
    assert call(op=smp.ctypes.data) == -1  # in place
    assert call(op=smp.ctypes.data + 8 * 4999) == -1 and call(sp=out.ctypes.data + 8 * 100) == -1  # overlapping
    dsmp = torch.zeros(5000 * ch + 8, dtype=torch.float32, device="cuda")
    dout = torch.zeros(5000 * ch + 8, dtype=torch.float32, device="cuda")
    dcnt = torch.tensor([0, 5000, 0, 0], dtype=torch.int32, device="cuda")
    doc = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # device pointers: samples and out aligned to a sample frame, the counts to an int
    assert call(sp=dsmp.data_ptr() + 4) == -1 and call(sp=dsmp.data_ptr() + 2) == -1
    assert call(op=dout.data_ptr() + 4) == -1 and call(op=dout.data_ptr() + 1) == -1
    assert call(cp=dcnt.data_ptr() + 2) == -1 and call(ocp=doc.data_ptr() + 1) == -1
    oc[0] = -7
    assert call() == 0 and oc[0] == 5000 and same_bits(out, smp)  # (the flat curve)
    assert call(mp3_amd.PACK_FLUSH, sp=dsmp.data_ptr() + 8, op=dout.data_ptr() + 8, cp=dcnt.data_ptr() + 4,
                ocp=doc.data_ptr() + 4) == 0
    dec.sync()
    assert doc.cpu().tolist() == [0, 5000, 0, 0]
    assert L.mp3d_batch_decode_equalized(dec._h, batch.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, 2, 1,
                                         out.ctypes.data, 5000, oc.ctypes.data, 4, None, None) == -1
    with pytest.raises(mp3_amd.MP3DError, match="-5"):
        dec.decode_equalized(batch.blob, offs[:2], sizes[:2], 2)  # more frames than the handle has


@pytest.mark.parametrize("fs,ch", [(48000, 2), (8000, 1)])
def test_host_and_device_buffers_agree(fs, ch):
    curve = "five_types"
    want = values(fs, ch, curve)
    xs = [x for _, _, x in _eq.streams(fs, ch)]
    n, ss = len(xs), max(_eq.LENGTHS)
    smp = torch.zeros((n, ss, ch), dtype=torch.float32, device="cuda")
    for s, x in enumerate(xs):
        smp[s, : len(x)] = torch.from_numpy(x.copy()).cuda()
    strm = torch.cuda.Stream()
    with torch.cuda.stream(strm):
        cnt = torch.tensor([len(x) for x in xs], dtype=torch.int32, device="cuda")
        out = torch.full((n, ss + 1, ch), float(PATTERN), dtype=torch.float32, device="cuda")
        oc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec = handle(n, fs, ch, curve)
        dec.eq(smp, cnt, out=out, out_counts=oc, stream=strm.cuda_stream)
    strm.synchronize()
    out, oc = out.cpu().numpy(), oc.cpu().numpy()
    assert list(oc) == [len(x) for x in xs]
    for s in range(n):
        assert same_bits(out[s, : oc[s]], want[s]) and (out[s, oc[s]:] == PATTERN).all(), s


def test_eq_time(batch):
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, "graphic", F=FS)
    offs, sizes = batch.geom(0, FS)
    dec.decode_equalized(batch.blob, offs, sizes, FS)
    with pytest.raises(mp3_amd.MP3DError):
        dec.eq_time_us()  # needs set_timing
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.eq_time_us()  # no equaliser call since
    dec.decode_equalized(batch.blob, offs, sizes, FS, flush=True)
    assert dec.eq_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- the debug builds -----------------------------------------------------------------------------
POISON_CASES = [(48000, 2, "graphic"), (11025, 1, "five_types")]


_plong = {}


def past_one_scan(fs, ch, curve):
    """one stream of 65 tiles and a little: the carry's second scan, on its poisoned scratch"""
    return feed(handle(1, fs, ch, curve), [_eq.signal("noise", fs, 65 * TILE + 5, ch, seed=65)])[0][0]


def product_results(fs, ch, curve):
    """the product library's results, without the poison: made before the caller's setenv"""
    if (fs, ch, curve) not in _plong:
        _plong[(fs, ch, curve)] = past_one_scan(fs, ch, curve)
    return values(fs, ch, curve), _plong[(fs, ch, curve)]


def assert_same_case(fs, ch, curve):
    want, want_long = product_results(fs, ch, curve)
    assert all(same_bits(a, b) for a, b in zip(run_values(fs, ch, curve), want))
    assert same_bits(past_one_scan(fs, ch, curve), want_long)


@pytest.mark.parametrize("fs,ch,curve", POISON_CASES)
def test_poison(fs, ch, curve, monkeypatch):
    product_results(fs, ch, curve)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    assert_same_case(fs, ch, curve)


@pytest.mark.parametrize("fs,ch,curve", POISON_CASES)
def test_workgroup_lds_poison_build(fs, ch, curve, monkeypatch):
    product_results(fs, ch, curve)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        assert_same_case(fs, ch, curve)
