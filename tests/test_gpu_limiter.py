"""GPU: the look-ahead true-peak limiter (BatchDecoder.set_limiter / limit /
decode_limited / decode_normalized(limit=True); include/mp3d.h "limiter").

Reference: the header's definition in numpy (tests/test_limiter_host.py
limit_ref: an exact float32 fmaf for the detector, float32 operations rounded
once and integers after it).  Every operation of the definition is exact
integer arithmetic or one float32 rounding, so every comparison here is on bits
and on exact counts; there is no tolerance.  One batch per format holds every
signal class at every length; its reference is computed once.

Measured, not asserted (test_true_peak_of_the_output prints it): the true peak
of the limiter's output over the ceiling, 20 log10(tp / c), per signal class
and format.  The gain moves between samples, so the oversampled peak of y may
pass c although no sample does.  On an MI355X, the largest over the lengths:
             quiet      impulses   burst      noise      edge_in / edge_out
  48 kHz x 2 -6.96 dB   +0.00008   +0.00003   +0.00055   -0.00000
  44.1 k x 2 -7.39 dB   +0.00009   +0.00004   +0.00075   -0.00000
  11 025 x 1 -6.85 dB   +0.00039   +0.00005   +0.00632   -0.00000
  8 kHz x 1  -7.14 dB   +0.00054   +0.00034   +0.00883   -0.00000
The largest is +0.0088 dB (uniform noise in +-2 at 8 kHz, where the look-ahead
is 80 samples and the gain moves fastest).  On decoded audio
(test_decode_normalized_with_the_limiter prints it): at most +0.0000 dB at
48 kHz stereo to -14 LUFS and +0.0010 dB at 11 025 Hz mono to -6 LUFS.
"""
import re

import numpy as np
import pytest
import torch

import mp3_amd
from mp3_amd import _build
from test_gpu_features import FS, Batch
from test_gpu_loudness import Tagged
from test_limiter_host import ceiling, int16_of, limit_ref, look

pytestmark = pytest.mark.gpu

FORMATS = [(48000, 2), (44100, 2), (11025, 1), (8000, 1)]
CLASSES = ["quiet", "impulses", "burst", "noise", "edge_in", "edge_out"]
DB = -1.0
PATTERN = np.float32(-777.25)
PATTERN16 = np.int16(-12345)
TILE = int(re.search(r"^#define MP3D_LIM_TILE\s+(\d+)", (_build.CSRC / "mp3d_limiter.h").read_text(), re.M).group(1))


def lens(fs):
    A = look(fs)
    return [0, 1, 5, 6, 7, A + 5, A + 6, A + 7, 4 * A + 11, 4 * A + 12, TILE - 1, TILE, TILE + A + 6, TILE + A + 7,
            3 * TILE + 17]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- signals and reference -------------------------------------------------------
def signal(fs, ch, name, n):
    """float32 [n, ch] of the class: the second channel differs from the first; nonzero magnitudes stay far above
    the denormals."""
    A = look(fs)
    rng = np.random.default_rng(811 + fs + ch + n)
    t = np.arange(n)
    x = np.zeros((n, ch))
    if name == "quiet":
        x = rng.uniform(-0.25, 0.25, (n, ch))
    elif name == "noise":
        x = rng.uniform(-2.0, 2.0, (n, ch))
    elif name == "burst":
        x = np.repeat((0.5 * np.sin(2.0 * np.pi * 440.0 * (t + 0.5) / fs))[:, None], ch, 1)
        x[n // 3: n // 3 + max(n // 10, 1)] *= 4.0
    else:
        at = {"impulses": [0, A - 1, n // 2, n - 1], "edge_in": [A + 7, 4 * A + 7],  # Hd + A apart: one window
              "edge_out": [A + 7, 4 * A + 8]}[name]  # Hd + A + 1 apart: no window holds both
        for k, i in enumerate(at):
            if 0 <= i < n:
                x[i] = 4.0 if k % 2 == 0 else -3.0
    if ch == 2:
        x[:, 1] *= -0.75
    return x.astype(np.float32)


_sig, _ref, _case = {}, {}, {}


def sig(fs, ch, name, n):
    key = (fs, ch, name, n)
    if key not in _sig:
        _sig[key] = signal(fs, ch, name, n)
        _sig[key].setflags(write=False)
    return _sig[key]


def ref(fs, ch, name, n, gain=None):
    """(y, g) of limit_ref on the class's signal: computed once, never changed."""
    key = (fs, ch, name, n, gain)
    if key not in _ref:
        y, g, _, _ = limit_ref(sig(fs, ch, name, n), fs, DB, gain)
        y.setflags(write=False), g.setflags(write=False)
        _ref[key] = (y, g)
    return _ref[key]


def emitted(fs, n, flush):
    return n if flush else max(n - look(fs) - 6, 0)


def gr_of(g, k):
    return np.float32(g[:k].min()) if k else np.float32(1.0)


def streams(fs):
    return [(c, n) for c in CLASSES for n in lens(fs)]


# ---- the stage -------------------------------------------------------------------
def handle(n, fs, ch, F=1, db=DB):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(fs, ch)
    dec.set_limiter(True, db)
    return dec


def feed(dec, xs, gain=None, flush=False, stride=None, f32=True):
    """Feed xs[s] ([k, ch]) to stream s in one call; returns ([output of s], counts, gr, raw out)."""
    n, (fs, ch) = len(xs), dec._out
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss, ch), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    cnt = np.array([len(x) for x in xs], np.int32)
    stride = stride if stride is not None else mp3_amd.limiter_max_samples(fs, ss)
    pat = PATTERN if f32 else PATTERN16
    out = np.full((n, stride, ch), pat, np.float32 if f32 else np.int16)
    gr = np.full(n, -5.0, np.float32)
    out, oc, gr = dec.limit(smp, cnt, gain, out=out, gr=gr, f32=f32, flush=flush)
    for s in range(n):
        assert (out[s, max(int(oc[s]), 0):] == pat).all(), s  # nothing past the count is touched
    return [out[s, : max(int(oc[s]), 0)].copy() for s in range(n)], oc, gr, out


def run_case(fs, ch):
    """{flush: (outputs, counts, gr)} of the format's batch, and the flushed int16 outputs"""
    xs = [sig(fs, ch, c, n) for c, n in streams(fs)]
    got = {flush: feed(handle(len(xs), fs, ch), xs, flush=flush)[:3] for flush in (True, False)}
    got[16] = feed(handle(len(xs), fs, ch), xs, flush=True, f32=False)[:3]
    return got


def case(fs, ch):
    if (fs, ch) not in _case:
        _case[(fs, ch)] = run_case(fs, ch)
    return _case[(fs, ch)]


@pytest.mark.parametrize("fs,ch", FORMATS)
@pytest.mark.parametrize("flush", [True, False])
def test_values(fs, ch, flush):
    """Every class at every length in one call: out, out_count and gr equal the reference bit for bit."""
    outs, oc, gr = case(fs, ch)[flush]
    limited = 0
    for s, (name, n) in enumerate(streams(fs)):
        what = "%d Hz x %d, %s, %d samples, flush %d" % (fs, ch, name, n, flush)
        y, g = ref(fs, ch, name, n)
        k = emitted(fs, n, flush)
        assert oc[s] == k, what
        assert same_bits(outs[s], y[:k]), what
        assert same_bits(gr[s], gr_of(g, k)), what
        if name == "quiet":
            assert same_bits(outs[s], sig(fs, ch, name, n)[:k]) and gr[s] == 1.0, what  # y == x
        limited += gr[s] < 1.0
    assert limited >= len(lens(fs)) // 2  # (the noise class alone, wherever the call emits anything)


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_int16_is_the_packed_sinks_rounding(fs, ch):
    outs, oc, gr = case(fs, ch)[16]
    f32 = case(fs, ch)[True]
    for s, (name, n) in enumerate(streams(fs)):
        assert oc[s] == n and outs[s].dtype == np.int16
        assert np.array_equal(outs[s], int16_of(f32[0][s])), (name, n)
        assert same_bits(gr[s], f32[2][s])


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_split_invariance(fs, ch):
    """The longest stream in calls of 1, A + 6, A + 7 and 997 samples with empty calls in between, another stream
    cut elsewhere in the neighbouring slot: the concatenation and the min-fold of gr are the one-call bits."""
    A = look(fs)
    n = lens(fs)[-1]
    names = ["noise", "burst"]
    xs = [sig(fs, ch, c, n) for c in names]
    sizes = [[1, 0, A + 6, 0, A + 7, 997, 0], [997, A + 7, 0, 1, 0, 0, A + 6]]
    dec = handle(2, fs, ch)
    pos, got, grs, i = [0, 0], [[], []], [[], []], 0
    while min(pos) < n:
        step = [min(sizes[s][i % 7], n - pos[s]) for s in (0, 1)]
        outs, oc, gr, _ = feed(dec, [xs[s][pos[s]: pos[s] + step[s]] for s in (0, 1)])
        for s in (0, 1):
            assert oc[s] == emitted(fs, pos[s] + step[s], False) - emitted(fs, pos[s], False), (s, i)
            got[s].append(outs[s]), grs[s].append(gr[s])
            if oc[s] == 0:
                assert gr[s] == 1.0
            pos[s] += step[s]
        i += 1
    outs, oc, gr, _ = feed(dec, [xs[0][:0], xs[1][:0]], flush=True)  # feeds nothing, emits the last A + 6
    for s in (0, 1):
        assert oc[s] == A + 6
        y, g = ref(fs, ch, names[s], n)
        assert same_bits(np.concatenate(got[s] + [outs[s]]), y), names[s]
        assert same_bits(min(grs[s] + [gr[s]]), gr_of(g, n)), names[s]
        assert same_bits(np.concatenate(got[s] + [outs[s]]), case(fs, ch)[True][0][streams(fs).index((names[s], n))])


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_pre_gain(fs, ch):
    n = TILE + look(fs) + 7
    x = sig(fs, ch, "burst", n)
    gains = [0.5, 1.0, 3.0]
    outs, oc, gr, _ = feed(handle(3, fs, ch), [x] * 3, gain=np.array(gains, np.float32), flush=True)
    for s, gv in enumerate(gains):
        y, g = ref(fs, ch, "burst", n, gv)
        assert oc[s] == n and same_bits(outs[s], y) and same_bits(gr[s], gr_of(g, n)), gv
    none, _, gr0, _ = feed(handle(1, fs, ch), [x], flush=True)  # gain NULL is gain 1
    assert same_bits(none[0], outs[1]) and same_bits(none[0], ref(fs, ch, "burst", n)[0]) and same_bits(gr0[0], gr[1])
    # the gain of the call that fed the sample: 0.5 then 3 is the stream 0.5 x | 3 x through one limiter
    cut = n // 2
    dec = handle(1, fs, ch)
    a, _, _, _ = feed(dec, [x[:cut]], gain=np.array([0.5], np.float32))
    b, _, _, _ = feed(dec, [x[cut:]], gain=np.array([3.0], np.float32), flush=True)
    v = np.concatenate([x[:cut] * np.float32(0.5), x[cut:] * np.float32(3.0)])
    assert same_bits(np.concatenate([a[0], b[0]]), limit_ref(v, fs, DB)[0])


def test_one_long_stream():
    """41 tiles at n_streams = 1: tiles are independent, one stream spreads over the GPU."""
    fs, ch = 48000, 2
    n = 40 * TILE + 3
    x = signal(fs, ch, "noise", n) * np.float32(0.3)
    x[::7919] *= np.float32(5.0)
    outs, oc, gr, _ = feed(handle(1, fs, ch), [x], flush=True)
    y, g, _, _ = limit_ref(x, fs, DB)
    assert oc[0] == n and -(-n // TILE) == 41
    assert same_bits(outs[0], y) and same_bits(gr[0], g.min()) and g.min() < 1.0 and (g == 1.0).any()


def test_true_peak_of_the_output():
    """Measured, not asserted: the true peak of the limiter's output over the ceiling, per class (the module
    docstring has the figures).  Asserted: no SAMPLE of any output is over c (1 + 2^-22)."""
    for fs, ch in FORMATS:
        outs, oc, _ = case(fs, ch)[True]
        c = ceiling(DB)
        dec = mp3_amd.BatchDecoder(len(outs), 1)
        dec.set_output(fs, ch)
        dec.set_true_peak(True)
        ss = max(len(o) for o in outs)
        smp = np.zeros((len(outs), ss, ch), np.float32)
        for s, o in enumerate(outs):
            smp[s, : len(o)] = o
        tp = dec.true_peak(smp, oc, flush=True)
        assert np.abs(smp).astype(np.float64).max() <= np.float64(c) * (1.0 + 2.0 ** -22)
        worst = {}
        for s, (name, n) in enumerate(streams(fs)):
            worst[name] = max(worst.get(name, 0.0), float(tp[s]))
        print("%d Hz x %d: true peak of the output over the ceiling, dB: " % (fs, ch)
              + ", ".join("%s %+.5f" % (k, 20.0 * np.log10(max(v, 1e-30) / c)) for k, v in worst.items()))


# ---- overflow and restarts -------------------------------------------------------
def test_stride_overflow():
    fs, ch = 44100, 2
    A = look(fs)
    a, b = 3 * A + 7, 2 * A
    x = sig(fs, ch, "noise", lens(fs)[-1])
    need = emitted(fs, a, False)
    dec = handle(3, fs, ch)
    outs, oc, gr, raw = feed(dec, [x[:a], x[:A], x[:a]], stride=need - 1)
    assert list(oc) == [-1, 0, -1] and list(gr) == [1.0, 1.0, 1.0]
    assert (raw == PATTERN).all()  # nothing written
    fresh, _, _, _ = feed(handle(1, fs, ch), [x[a:a + b]])
    cont = handle(1, fs, ch)
    feed(cont, [x[:A]])
    second, _, _, _ = feed(cont, [x[a:a + b]])
    nxt, nc, _, _ = feed(dec, [x[a:a + b]] * 3)
    assert same_bits(nxt[0], fresh[0]) and same_bits(nxt[2], fresh[0])  # the two were restarted
    assert same_bits(nxt[1], second[0]) and not same_bits(second[0][: len(fresh[0])], fresh[0])  # the third goes on
    outs, oc, _, _ = feed(handle(1, fs, ch), [x[:a]], stride=need)  # exactly the need fits
    assert list(oc) == [need]
    outs, oc, _, _ = feed(handle(1, fs, ch), [x[:a]], stride=a - 1, flush=True)
    assert list(oc) == [-1]


def test_restarts():
    """Every restart of the definition: the slot then answers as a fresh one does, and the others go on."""
    fs, ch = 11025, 1
    A = look(fs)
    x = sig(fs, ch, "noise", lens(fs)[-1])
    a, b = 2 * A + 3, 5 * A + 1
    fresh, _, _, _ = feed(handle(1, fs, ch), [x[a:a + b]])
    cont = handle(1, fs, ch)
    feed(cont, [x[:a]])
    goes_on, _, _, _ = feed(cont, [x[a:a + b]])
    assert len(goes_on[0]) == b and len(fresh[0]) == b - A - 6

    def primed(n=2):
        dec = handle(n, fs, ch)
        feed(dec, [x[:a]] * n)
        return dec

    def expect(dec, restarted):
        outs, oc, _, _ = feed(dec, [x[a:a + b]] * len(restarted))
        for s, r in enumerate(restarted):
            assert same_bits(outs[s], fresh[0] if r else goes_on[0]), (s, r)

    expect(primed(), [False, False])
    dec = primed()
    dec.reset()
    expect(dec, [True, True])
    dec = primed()
    dec.set_state(dec.get_state()[1:2], first=1)
    expect(dec, [False, True])
    dec = primed()
    dec.set_window([0], first=0)
    expect(dec, [True, False])
    dec = primed()
    dec.set_limiter(True, DB)
    expect(dec, [True, True])
    dec = primed()
    dec.set_output(fs, ch)  # turns the limiter off
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        feed(dec, [x[:a]] * 2)
    dec.set_limiter(True, DB)
    expect(dec, [True, True])
    dec = primed()
    tail, oc, _, _ = feed(dec, [x[:0], x[:7]], flush=True)  # its own flush restarts both
    assert list(oc) == [A + 6, A + 6 + 7]
    expect(dec, [True, True])
    # the other sinks' states are not the limiter's: a true-peak call in between changes nothing
    dec = primed()
    dec.set_true_peak(True)
    dec.true_peak(np.ascontiguousarray(x[None, :a]), [a])
    expect(dec, [False, False])


def test_argument_errors(batch):
    fs, ch = 48000, 2
    L = mp3_amd.lib()
    x = np.ascontiguousarray(sig(fs, ch, "noise", 5000)[None])
    dec = mp3_amd.BatchDecoder(2, 1)
    assert L.mp3d_batch_set_limiter(dec._h, 1, -1.0) == -1  # no packed format yet
    dec.set_output(fs, ch)
    cnt, oc = np.array([5000, 0], np.int32), np.zeros(2, np.int32)
    out = np.zeros((2, 6000, ch), np.float32)

    def call(flags=0, n=1, sp=x.ctypes.data, op=out.ctypes.data, cp=cnt.ctypes.data, ocp=oc.ctypes.data, gp=None,
             rp=None, stride=5000, ostride=6000, f32=1):
        return L.mp3d_batch_limit(dec._h, sp, stride, cp, n, gp, op, f32, ostride, ocp, rp, flags, None)

    assert call() == -1  # before set_limiter
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.limit(x, [5000])
    offs, sizes = batch.geom(0, 1)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_limited(batch.blob, offs[:2], sizes[:2], 1)
    for db in (0.001, -20.001, float("nan"), float("inf")):
        assert L.mp3d_batch_set_limiter(dec._h, 1, db) == -1, db
    assert call() == -1  # a refused ceiling leaves the limiter off
    assert L.mp3d_batch_set_limiter(dec._h, 1, -20.0) == 0 and L.mp3d_batch_set_limiter(dec._h, 1, 0.0) == 0
    dec.set_limiter(True, DB)
    assert call(4) == -1 and call(mp3_amd.PACK_GAPLESS) == -1  # unknown flag; the stage has no frames to read a tag from
    assert call(n=3) == -5 and call(n=0) == -1
    assert call(sp=None) == -1 and call(op=None) == -1 and call(cp=None) == -1 and call(ocp=None) == -1
    assert call(stride=-1) == -1 and call(ostride=-1) == -1 and call(stride=2 ** 31 - 1) == -1
    dsmp = torch.zeros(2 * 5000 * ch + 4, dtype=torch.float32, device="cuda")
    dout = torch.zeros(2 * 6000 * ch + 8, dtype=torch.float32, device="cuda")
    dcnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    dgn = torch.ones(4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert call(sp=dsmp.data_ptr() + 2) == -1  # misaligned device pointers
    assert call(op=dout.data_ptr() + 4) == -1  # a device out is aligned to one sample frame
    assert call(op=dout.data_ptr() + 2, f32=0) == -1  # (of int16 too)
    assert call(ocp=dcnt.data_ptr() + 2) == -1 and call(cp=dcnt.data_ptr() + 1) == -1
    assert call(gp=dgn.data_ptr() + 2) == -1 and call(rp=dgn.data_ptr() + 1) == -1
    assert call(sp=dsmp.data_ptr(), op=dsmp.data_ptr(), ostride=5000) == -1  # out overlapping samples
    assert call(sp=dsmp.data_ptr(), op=dsmp.data_ptr() + 4 * 5000 * ch - 8, ostride=100) == -1
    assert call(sp=x.ctypes.data, op=x.ctypes.data, ostride=5000) == -1
    assert call(sp=dsmp.data_ptr() + 4, op=dout.data_ptr() + 8, ocp=dcnt.data_ptr() + 4, gp=dgn.data_ptr() + 4,
                rp=dgn.data_ptr() + 8) == 0
    assert call(mp3_amd.PACK_FLUSH) == 0
    dec.sync()

    def decode(flags=0, n=2, F=1, op=out.ctypes.data, ocp=oc.ctypes.data):
        return L.mp3d_batch_decode_limited(dec._h, batch.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, n, F,
                                           None, op, 1, 6000, ocp, None, flags, None, None)

    assert decode(4) == -1 and decode(op=None) == -1 and decode(ocp=None) == -1 and decode(n=3) == -5
    assert decode(F=2) == -5 and decode(n=0) == -1
    assert decode(mp3_amd.PACK_FLUSH | mp3_amd.PACK_GAPLESS) == 0
    # decode_normalized(limit=True) wants the limiter, at its ceiling
    dec.set_loudness(True)
    dec.set_true_peak(True)
    with pytest.raises(mp3_amd.MP3DError, match="ceiling"):
        dec.decode_normalized(batch.blob, offs[:2], sizes[:2], 1, max_dbtp=-2.0, limit=True)
    dec.set_limiter(False)
    with pytest.raises(mp3_amd.MP3DError, match="set_limiter"):
        dec.decode_normalized(batch.blob, offs[:2], sizes[:2], 1, limit=True)


@pytest.mark.parametrize("fs,ch", [(48000, 2), (8000, 1)])
def test_host_and_device_buffers_agree(fs, ch):
    st = [(c, n) for c, n in streams(fs) if n >= TILE - 1 and c in ("noise", "burst", "impulses")]
    base = [streams(fs).index(k) for k in st]
    n, ss = len(st), lens(fs)[-1]
    smp = torch.zeros((n, ss, ch), dtype=torch.float32, device="cuda")
    for s, (name, k) in enumerate(st):
        smp[s, :k] = torch.from_numpy(sig(fs, ch, name, k).copy()).cuda()
    stride = mp3_amd.limiter_max_samples(fs, ss)
    strm = torch.cuda.Stream()
    for flush in (True, False):
        want, wc, wgr = case(fs, ch)[flush]
        with torch.cuda.stream(strm):
            cnt = torch.tensor([k for _, k in st], dtype=torch.int32, device="cuda")
            out = torch.full((n, stride, ch), float(PATTERN), dtype=torch.float32, device="cuda")
            got = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            gr = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dec = handle(n, fs, ch)
            dec.limit(smp, cnt, out=out, out_counts=got, gr=gr, flush=flush, stream=strm.cuda_stream)
        strm.synchronize()
        out, got, gr = out.cpu().numpy(), got.cpu().numpy(), gr.cpu().numpy()
        for s in range(n):
            w = want[base[s]]
            assert got[s] == len(w) and same_bits(out[s, : got[s]], w) and (out[s, got[s]:] == PATTERN).all()
            assert same_bits(gr[s], wgr[base[s]])
        mixed, mc, mgr = handle(n, fs, ch).limit(smp, cnt, flush=flush)  # device in, host out
        for s in range(n):
            assert mc[s] == got[s] and same_bits(mixed[s, : mc[s]], out[s, : got[s]]) and same_bits(mgr[s], gr[s])


# ---- composition -----------------------------------------------------------------
DEC_FMT = (48000, 2)


@pytest.fixture(scope="module")
def batch():
    return Tagged(Batch())


def batch_gains(n):
    return np.array([[0.5, 1.0, 4.0, 9.0][s % 4] for s in range(n)], np.float32)


def packed(batch, gapless=False):
    fs, ch = DEC_FMT
    dec = mp3_amd.BatchDecoder(batch.n, FS)
    dec.set_output(fs, ch)
    offs, sizes = batch.geom(0, FS)
    return dec.decode_packed(batch.blob, offs, sizes, FS, flush=True, gapless=gapless)[:2]


def decode_chunks(batch, chunks=(FS,), gapless=False, f32=True):
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, F=max(chunks))
    got, grs, a = [[] for _ in range(batch.n)], [], 0
    for i, c in enumerate(chunks):
        offs, sizes = batch.geom(a, a + c)
        stride = mp3_amd.limiter_max_samples(fs, mp3_amd.packed_max_samples(fs, c))
        pat = PATTERN if f32 else PATTERN16
        out = np.full((batch.n, stride, ch), pat, np.float32 if f32 else np.int16)
        out, oc, gr, _ = dec.decode_limited(batch.blob, offs, sizes, c, gain=batch_gains(batch.n), out=out, f32=f32,
                                            flush=i == len(chunks) - 1, gapless=gapless)
        for s in range(batch.n):
            assert oc[s] >= 0 and (out[s, oc[s]:] == pat).all()
            got[s].append(out[s, : oc[s]].copy())
        grs.append(gr.copy())
        a += c
    return [np.concatenate(g) for g in got], np.min(grs, axis=0)


@pytest.mark.parametrize("gapless", [False, True])
def test_decode_limited_is_the_stage_on_the_packed_samples(batch, gapless):
    fs, ch = DEC_FMT
    smp, counts = packed(batch, gapless)
    via, oc, vgr, _ = feed(handle(batch.n, fs, ch), [smp[s, : counts[s]] for s in range(batch.n)],
                           gain=batch_gains(batch.n), flush=True)
    assert oc[batch.names.index("empty")] == 0 and np.array_equal(oc, counts)
    one, gr1 = decode_chunks(batch, gapless=gapless)
    two, gr2 = decode_chunks(batch, (5, 11), gapless=gapless)
    for s in range(batch.n):
        assert same_bits(one[s], via[s]) and same_bits(two[s], via[s]), batch.names[s]
    assert same_bits(gr1, vgr) and same_bits(gr2, vgr) and (vgr < 1.0).any() and (vgr == 1.0).any()
    for s in (0, 2):  # and the definition itself, on decoded audio
        assert same_bits(via[s], limit_ref(smp[s, : counts[s]], fs, DB, float(batch_gains(batch.n)[s]))[0])
    if not gapless:
        i16, _ = decode_chunks(batch, (5, 11), f32=False)
        for s in range(batch.n):
            assert np.array_equal(i16[s], int16_of(via[s])), batch.names[s]


def normalizer(batch, fs, ch, limiter):
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    dec.set_output(fs, ch)
    dec.set_loudness(True)
    dec.set_true_peak(True)
    if limiter:
        dec.set_limiter(True, DB)
    return dec


@pytest.mark.parametrize("fs,ch,target", [(48000, 2, -14.0), (11025, 1, -6.0)])
def test_decode_normalized_with_the_limiter(batch, fs, ch, target):
    F = batch.F
    offs, sizes = batch.geom()
    out, counts, lufs, tp, gain, infos = normalizer(batch, fs, ch, True).decode_normalized(
        batch.blob, offs, sizes, F, target=target, max_dbtp=DB, limit=True)
    # the composition, call by call
    dec = normalizer(batch, fs, ch, True)
    smp, cnt, winfos = dec.decode_packed(batch.blob, offs, sizes, F, flush=True)
    blocks, bc, _ = dec.loudness(smp, cnt, flush=True)
    wtp = dec.true_peak(smp, cnt, flush=True)
    wl = dec.integrated_lufs(blocks, bc)
    wg = dec.normalize_gain(wl, None, target=target, max_dbtp=DB)  # no cap
    want, wc, wgr = dec.limit(smp, cnt, wg, flush=True, stride=smp.shape[1])
    assert np.array_equal(counts, cnt) and np.array_equal(wc, cnt) and np.array_equal(infos, winfos)
    assert same_bits(lufs, wl) and same_bits(tp, wtp) and same_bits(gain, wg) and same_bits(out, want)
    out16 = normalizer(batch, fs, ch, True).decode_normalized(batch.blob, offs, sizes, F, target=target, max_dbtp=DB,
                                                              f32=False, limit=True)[0]
    assert out16.dtype == np.int16 and np.array_equal(out16, int16_of(out))
    # every stream with a loudness got the uncapped gain, the limiter acted on some, and no sample is over the ceiling
    c = ceiling(DB)
    fin = np.isfinite(lufs)
    assert fin.any() and (gain[~fin] == 1.0).all()
    # The limiter acts exactly where today's rule would have turned the stream down: the largest detector value of
    # the stream fl(x g) is g tpeak up to the roundings of two 12-term chains and one multiply (23 * 2^-24 of the
    # peak each side, the tap's contract, and 2^-24: under 3e-6 together), so outside a band of 1e-5 around the
    # ceiling gr < 1 and g tpeak > c say the same.
    peak = wg.astype(np.float64) * wtp
    for s in range(batch.n):
        if peak[s] > c * (1.0 + 1e-5):
            assert wgr[s] < 1.0, (batch.names[s], peak[s])
        elif peak[s] < c * (1.0 - 1e-5):
            assert wgr[s] == 1.0, (batch.names[s], peak[s])
    capped = peak[fin] > c
    print("%d of %d streams with a loudness pass the ceiling at the uncapped gain, the limiter acted on %d"
          % (capped.sum(), fin.sum(), (wgr[fin] < 1.0).sum()))
    if target > -10.0:  # (so loud that no programme material fits under the ceiling)
        assert capped.any() and (wgr[fin] < 1.0).any()
    assert np.abs(out).astype(np.float64).max() <= np.float64(c) * (1.0 + 2.0 ** -22)
    blocks, bc, _ = dec.loudness(out, counts, flush=True)
    after = dec.integrated_lufs(blocks, bc)
    tp_after = dec.true_peak(out, counts, flush=True)
    print("decode_normalized(limit=True) %d Hz x %d to %g LUFS: lufs after - target %s; true peak after over the "
          "ceiling, dB %s" % (fs, ch, target, np.round(after[fin] - target, 3),
                               np.round(20.0 * np.log10(np.maximum(tp_after[fin], 1e-30) / c), 4)))


@pytest.mark.parametrize("fs,ch,target", [(48000, 2, -16.0)])
def test_decode_normalized_without_the_keyword_is_unchanged(batch, fs, ch, target):
    """limit defaults to False: today's sequence of calls, whether or not the limiter is set.  The comparison is
    with that sequence made call by call on this build (decode_packed, loudness, true_peak, integrated_lufs,
    normalize_gain with tpeak, apply_gain), which is what decode_normalized is defined as and what
    tests/test_gpu_normalize.py pins it to; no result recorded from an earlier build is read."""
    F = batch.F
    offs, sizes = batch.geom()
    dec = normalizer(batch, fs, ch, False)
    smp, cnt, winfos = dec.decode_packed(batch.blob, offs, sizes, F, flush=True)
    blocks, bc, _ = dec.loudness(smp, cnt, flush=True)
    wtp = dec.true_peak(smp, cnt, flush=True)
    wl = dec.integrated_lufs(blocks, bc)
    wg = dec.normalize_gain(wl, wtp, target=target, max_dbtp=DB)
    want = dec.apply_gain(smp, cnt, wg)
    for limiter in (False, True):
        out, counts, lufs, tp, gain, infos = normalizer(batch, fs, ch, limiter).decode_normalized(
            batch.blob, offs, sizes, F, target=target, max_dbtp=DB)
        assert np.array_equal(counts, cnt) and np.array_equal(infos, winfos)
        assert same_bits(lufs, wl) and same_bits(tp, wtp) and same_bits(gain, wg) and same_bits(out, want)


def test_limited_samples_feed_the_other_stages():
    """limit's device out and counts into true_peak() and apply_gain()."""
    fs, ch = 48000, 2
    n = TILE + 100
    x = sig(fs, ch, "burst", n)
    dec = handle(1, fs, ch)
    dec.set_true_peak(True)
    smp = torch.from_numpy(x.copy()[None]).cuda()
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    out = torch.zeros((1, mp3_amd.limiter_max_samples(fs, n), ch), dtype=torch.float32, device="cuda")
    oc = torch.zeros(1, dtype=torch.int32, device="cuda")
    gr = torch.zeros(1, dtype=torch.float32, device="cuda")
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dec.limit(smp, cnt, out=out, out_counts=oc, gr=gr, flush=True)
    tp = dec.true_peak(out, oc, flush=True)
    i16 = dec.apply_gain(out, oc, one, f32=False)
    dec.sync()
    y = ref(fs, ch, "burst", n)[0]
    host = mp3_amd.BatchDecoder(1, 1)
    host.set_output(fs, ch)
    host.set_true_peak(True)
    assert same_bits(tp, host.true_peak(np.ascontiguousarray(y[None]), [n], flush=True))
    assert np.array_equal(i16[0, :n], int16_of(y))


def test_limiter_time(batch):
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, F=FS)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.limiter_time_us()  # no limiter call yet
    offs, sizes = batch.geom(0, FS)
    dec.decode_limited(batch.blob, offs, sizes, FS, flush=True)
    assert dec.limiter_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- poison ----------------------------------------------------------------------
def assert_same_case(fs, ch):
    got, want = run_case(fs, ch), case(fs, ch)
    for key in want:
        for g, w in zip(got[key][0], want[key][0]):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), key
        assert np.array_equal(got[key][1], want[key][1]) and same_bits(got[key][2], want[key][2]), key


def test_poison(monkeypatch):
    fs, ch = 48000, 2
    case(fs, ch)  # (the product library's, without the poison)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    assert_same_case(fs, ch)


def test_workgroup_lds_poison_build(monkeypatch):
    fs, ch = 11025, 1
    case(fs, ch)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        assert_same_case(fs, ch)
