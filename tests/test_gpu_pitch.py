"""GPU: the pitch sink (BatchDecoder.set_pitch / pitch / decode_pitch /
long_pitch; include/mp3d.h "pitch sink").

Reference: the header's definition in numpy (tests/test_pitch_host.py pitch_ref
and pitch_by_call).  lag and shift are integers and must be equal; f0_hz and
periodicity are single correctly rounded double operations on exact integers,
so equality is expected and one float32 ulp is allowed for a compiler that
reorders; differing() counts the records that differ at all.  Between two runs
of the GPU (splits, buffers, builds) the comparison is on bytes.
"""
import re

import numpy as np
import pytest
import torch

import mp3_amd
from mp3_amd import _build
from test_gpu_features import FS, Batch
from test_pitch_host import DT, harmonic, hop, known, lags, pitch_by_call, pitch_ref, quantise, same

pytestmark = pytest.mark.gpu

FORMATS = [(16000, 1), (48000, 2), (44100, 2), (22050, 1), (8000, 1)]
PATTERN = 0xAB
TILE = int(re.search(r"^#define MP3D_PT_TILE\s+(\d+)", (_build.CSRC / "mp3d_pitch.h").read_text(), re.M).group(1))


def params(fs):
    return [(60, 500, 154), (50, min(fs // 4, 2000), 154), (50, 400, 1024), (200, 300, 1)]


# ---- comparison -------------------------------------------------------------------
def ulps(a, b):
    a, b = (np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(a - b)  # (both are >= 0: the sign bit never differs)


def differing(got, want, what=""):
    """asserts the comparison rule; returns the number of records that differ at all"""
    assert got.shape == want.shape, what
    assert np.array_equal(got["lag"], want["lag"]) and np.array_equal(got["shift"], want["shift"]), what
    for k in ("f0_hz", "periodicity"):
        assert (got[k] >= 0).all() and (ulps(got[k], want[k]) <= 1).all(), (what, k)
    return int(sum(g.tobytes() != w.tobytes() for g, w in zip(got, want)))


# ---- signals ----------------------------------------------------------------------
def stereo(x, ch):
    """[n] -> [n, ch]; in stereo the channels differ by 0.5 and only their float32 mix carries the signal"""
    x = np.asarray(x, np.float32)
    return x[:, None] if ch == 1 else np.stack([x + np.float32(0.25), x - np.float32(0.25)], axis=1)


def tone(fs, f, n, amp=0.5):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / fs)).astype(np.float32)


def streams(fs, ch, fmin, fmax):
    """[(name, x float32 [n, ch])] of one case's batch"""
    H = hop(fs)
    tmin, tmax, SPAN = lags(fs, fmin, fmax)
    n = SPAN + H
    rng = np.random.default_rng(fs + ch + fmin + fmax)
    per = 2 * max(tmin // 2 + 1, 2)  # an even period: D(per) = D(2 per) = 0 exactly
    sq = np.where(np.arange(n) % per < per // 2, 0.25, -0.25)
    click = tone(fs, 0.5 * (fmin + fmax), n, 0.004)
    click[n // 2] = -1.0
    f = 0.5 * (fmin + min(fmax, 4 * fmin))
    out = [("tone_tmin", tone(fs, fs / tmin, n)), ("tone_tmax", tone(fs, fs / max(tmax, 1), n)),
           ("harmonic", harmonic(fs, f, n)), ("missing", harmonic(fs, f, n, missing=True)),
           ("glide", (0.5 * np.sin(2 * np.pi * np.cumsum(np.linspace(fmin, fmax, n)) / fs)).astype(np.float32)),
           ("noise", rng.uniform(-0.5, 0.5, n)), ("zeros", np.zeros(n)), ("dc_min", np.full(n, -1.0)),
           ("alternation", np.where(np.arange(n) % 2 == 0, 1.0, -1.0)), ("square", sq), ("click", click)]
    for k in (0, 1, H - 1, SPAN - 1, SPAN, SPAN + H - 1, SPAN + H, fs // 2):
        out.append(("len_%d" % k, harmonic(fs, f, max(k, 1), seed=k)[:k]))
    return [(name, stereo(x, ch)) for name, x in out]


_streams, _ref, _case = {}, {}, {}


def batch_of(fs, ch, fmin, fmax):
    key = (fs, ch, fmin, fmax)
    if key not in _streams:
        _streams[key] = streams(fs, ch, fmin, fmax)
        for _, x in _streams[key]:
            x.setflags(write=False)
    return _streams[key]


def ref(fs, ch, fmin, fmax, theta, flush):
    """[records of stream s] of the batch fed to fresh slots in one call: computed once, never changed (the
    frames known without a flush are the first of the flushed stream's)"""
    key = (fs, ch, fmin, fmax, theta)
    if key not in _ref:
        _ref[key] = [pitch_ref(quantise(x), fs, fmin, fmax, theta, True) for _, x in batch_of(fs, ch, fmin, fmax)]
    if flush:
        return _ref[key]
    H, SPAN = hop(fs), lags(fs, fmin, fmax)[2]
    return [r[: known(len(x), H, SPAN)] for r, (_, x) in zip(_ref[key], batch_of(fs, ch, fmin, fmax))]


# ---- the stage --------------------------------------------------------------------
def handle(n, fs, ch, fmin=60, fmax=500, theta=154, F=1):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(fs, ch)
    dec.set_pitch(True, fmin, fmax, theta / 1024.0)
    return dec


def feed(dec, xs, flush=False, stride=None):
    """Feed xs[s] ([k, ch]) to stream s in one call; returns ([records of s], counts, raw out)."""
    n, (fs, ch) = len(xs), dec._out
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss, ch), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    cnt = np.array([len(x) for x in xs], np.int32)
    stride = stride if stride is not None else mp3_amd.pitch_max_frames(fs, ss, dec._pitch)
    out = np.full((n, stride, 16), PATTERN, np.uint8).view(DT).reshape(n, stride)
    out, oc = dec.pitch(smp, cnt, out=out, flush=flush)
    for s in range(n):
        assert (out[s, max(int(oc[s]), 0):].view(np.uint8) == PATTERN).all(), s  # nothing past the count is touched
    return [out[s, : max(int(oc[s]), 0)].copy() for s in range(n)], oc, out


def run_case(fs, ch, fmin, fmax, theta):
    """{flush: (records, counts)} of the batch in one call on fresh slots"""
    xs = [x for _, x in batch_of(fs, ch, fmin, fmax)]
    return {flush: feed(handle(len(xs), fs, ch, fmin, fmax, theta), xs, flush=flush)[:2] for flush in (True, False)}


def case(fs, ch, fmin, fmax, theta):
    key = (fs, ch, fmin, fmax, theta)
    if key not in _case:
        _case[key] = run_case(*key)
    return _case[key]


@pytest.mark.parametrize("fs,ch", FORMATS)
@pytest.mark.parametrize("pi", range(4))
def test_values(fs, ch, pi):
    """Every signal and stream length in one call, flushed and not, against the definition."""
    fmin, fmax, theta = params(fs)[pi]
    H = hop(fs)
    tmin, tmax, SPAN = lags(fs, fmin, fmax)
    names = [k for k, _ in batch_of(fs, ch, fmin, fmax)]
    diff = 0
    for flush in (True, False):
        got, oc = case(fs, ch, fmin, fmax, theta)[flush]
        want = ref(fs, ch, fmin, fmax, theta, flush)
        for s, name in enumerate(names):
            what = "%d Hz x %d, %d..%d Hz theta %d, %s, flush %d" % (fs, ch, fmin, fmax, theta, name, flush)
            assert oc[s] == len(want[s]), what
            diff += differing(got[s], want[s], what)
    print("pitch records that differ from the reference at all: %d" % diff)
    # what the signals are there to show, on the flushed records' first frame (it reads no zeros behind the end)
    w = {k: r for k, r in zip(names, ref(fs, ch, fmin, fmax, theta, True))}
    assert not w["zeros"]["lag"].any() and not w["dc_min"]["lag"].any() and w["dc_min"]["shift"][0] == 6
    assert w["click"]["shift"][0] == 6 and w["alternation"]["shift"][0] == 6
    assert w["harmonic"]["shift"][0] in (4, 5)  # (a peak of 0.5 quantises to 16384 or, through the stereo mix, just under)
    assert len(w["len_0"]) == 0 and len(w["len_%d" % SPAN]) == -(-SPAN // H)
    assert len(ref(fs, ch, fmin, fmax, theta, False)[names.index("len_%d" % (SPAN - 1))]) == 0
    assert len(ref(fs, ch, fmin, fmax, theta, False)[names.index("len_%d" % SPAN)]) == 1
    if theta == 154 and tmin <= tmax:
        assert w["noise"]["lag"][0] == 0 and w["harmonic"]["lag"][0] > 0 and w["missing"]["lag"][0] > 0
    if theta == 1024 and ch == 1 and tmin <= tmax:
        per = 2 * max(tmin // 2 + 1, 2)
        assert w["square"]["lag"][0] == per  # the tie with 2 per goes to the smaller lag


def cuts_of(n, sizes):
    cuts, pos, i = [], 0, 0
    while pos < n:
        pos = min(pos + sizes[i % len(sizes)], n)
        cuts.append(pos)
        i += 1
    return cuts + [n]  # the last call feeds nothing and flushes


@pytest.mark.parametrize("fs,ch", [(16000, 1), (44100, 2)])
def test_split_invariance(fs, ch):
    """Two streams in calls of 1, H - 1, H, SPAN - 1, SPAN and random sizes with empty calls in between, cut at
    different places: each call emits the records the emit rule assigns to it, the single call's bytes."""
    H = hop(fs)
    SPAN = lags(fs, 60, 500)[2]
    rng = np.random.default_rng(fs)
    n = 4 * SPAN + 3 * H + 5
    xs = [stereo(harmonic(fs, f, n, seed=int(f)), ch) for f in (123.0, 311.0)]
    sizes = [[1, 0, H - 1, H, SPAN - 1, int(rng.integers(1, SPAN)), SPAN, 0],
             [SPAN, int(rng.integers(1, SPAN)), 0, 1, H, 0, H - 1, SPAN - 1]]
    cuts = [cuts_of(n, z) for z in sizes]
    ncall = max(len(c) for c in cuts)
    cuts = [c + [n] * (ncall - len(c)) for c in cuts]
    whole, wc, _ = feed(handle(2, fs, ch), xs, flush=True)
    want = [pitch_by_call(quantise(xs[s]), fs, 60, 500, 154, cuts[s], True) for s in (0, 1)]
    dec = handle(2, fs, ch)
    at, total = [0, 0], [[], []]
    for i in range(ncall):
        got, oc, _ = feed(dec, [xs[s][at[s]: cuts[s][i]] for s in (0, 1)], flush=i == ncall - 1)
        for s in (0, 1):
            assert oc[s] == len(want[s][i]), (s, i)
            differing(got[s], want[s][i], (s, i))
            total[s].append(got[s])
            at[s] = cuts[s][i]
    for s in (0, 1):
        assert same(np.concatenate(total[s]), whole[s]) and len(whole[s]) == -(-n // H)
        assert sum(len(w) > 0 for w in want[s][:-1]) > 3  # records come out along the way


def test_every_alignment_of_a_call_boundary():
    """Calls of H + 1 samples: the boundary walks through every offset inside a frame, odd and even."""
    fs, ch = 8000, 1
    H = hop(fs)
    n = H * (H + 1)
    x = stereo(harmonic(fs, 97.0, n), ch)
    whole, _, _ = feed(handle(1, fs, ch), [x], flush=True)
    dec = handle(1, fs, ch)
    parts = [feed(dec, [x[a: a + H + 1]], flush=a + H + 1 >= n)[0][0] for a in range(0, n, H + 1)]
    assert {a % H for a in range(0, n, H + 1)} == set(range(H))
    assert same(np.concatenate(parts), whole[0]) and len(whole[0]) == H + 1
    assert differing(whole[0], pitch_ref(quantise(x), fs, 60, 500, 154, True)) >= 0


@pytest.mark.parametrize("fs,ch,shift", [(48000, 2, 2), (48000, 2, 1), (44100, 2, 3), (22050, 1, 1), (8000, 1, 3)])
def test_strided_input(fs, ch, shift):
    """Samples that start `shift` floats into their allocation, rows an odd stride apart."""
    SPAN = lags(fs, 60, 500)[2]
    xs = [stereo(harmonic(fs, 100.0 + 40 * r, SPAN + (2 + r) * hop(fs) + r, seed=r), ch) for r in (0, 1, 2)]
    ss = max(len(x) for x in xs) + 1
    flat = torch.zeros(shift + 3 * ss * ch, dtype=torch.float32, device="cuda")
    smp = flat[shift:].view(3, ss, ch)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    assert smp.data_ptr() == flat.data_ptr() + 4 * shift
    out, oc = handle(3, fs, ch).pitch(smp, [len(x) for x in xs], flush=True)
    for s, x in enumerate(xs):
        want = pitch_ref(quantise(x), fs, 60, 500, 154, True)
        assert oc[s] == len(want) > 3
        differing(out[s, : oc[s]], want, s)


def test_one_long_stream():
    """3 s at n_streams = 1 on device memory: frames are independent, one stream spreads over the GPU."""
    fs, ch = 48000, 2
    n = 3 * fs + 17
    f = np.linspace(90.0, 240.0, n)
    x = stereo((0.4 * np.sin(2 * np.pi * np.cumsum(f) / fs) + 0.1 * np.sin(4 * np.pi * np.cumsum(f) / fs)), ch)
    smp = torch.from_numpy(x[None].copy()).cuda()
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    stride = mp3_amd.pitch_max_frames(fs, n, 60)
    out = torch.full((1, stride, 4), -1, dtype=torch.int32, device="cuda")
    oc = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec = handle(1, fs, ch)
    dec.pitch(smp, cnt, out=out, out_counts=oc, flush=True)
    dec.sync()
    k = int(oc.cpu()[0])
    want = pitch_ref(quantise(x), fs, 60, 500, 154, True)
    assert k == len(want) == -(-n // hop(fs)) and -(-k // TILE) > 1
    got = out.cpu().numpy().view(DT).reshape(1, stride)[0]
    print("pitch records that differ from the reference at all: %d" % differing(got[:k], want))
    assert (got[k:].view(np.int32) == -1).all() and (want["lag"] > 0).mean() > 0.9


# ---- overflow and restarts --------------------------------------------------------
def test_stride_overflow():
    fs, ch = 22050, 1
    H, SPAN = hop(fs), lags(fs, 60, 500)[2]
    a = stereo(harmonic(fs, 140.0, SPAN + 3 * H), ch)  # four frames without a flush
    short = a[: SPAN - 1]  # nothing emitted yet
    b = stereo(harmonic(fs, 190.0, SPAN + H, seed=5), ch)
    dec = handle(3, fs, ch)
    got, oc, raw = feed(dec, [a, short, a], stride=3)
    assert list(oc) == [-1, 0, -1] and (raw.view(np.uint8) == PATTERN).all()  # nothing written
    fresh = feed(handle(1, fs, ch), [b])[0][0]
    cont = handle(1, fs, ch)
    feed(cont, [short])
    second = feed(cont, [b])[0][0]
    nxt, _, _ = feed(dec, [b] * 3)
    assert same(nxt[0], fresh) and same(nxt[2], fresh) and len(fresh) == 2  # the two were restarted
    assert same(nxt[1], second) and len(second) > len(fresh)  # the third goes on
    assert list(feed(handle(1, fs, ch), [a], stride=4)[1]) == [4]  # exactly the need fits
    assert list(feed(handle(1, fs, ch), [a], stride=0)[1]) == [-1]


def test_restarts():
    """Every restart of the definition: the slot then answers as a fresh one does, the others go on."""
    fs, ch = 11025, 1
    H, SPAN = hop(fs), lags(fs, 60, 500)[2]
    a = stereo(harmonic(fs, 140.0, SPAN + H + 7), ch)
    b = stereo(harmonic(fs, 190.0, SPAN + H, seed=5), ch)
    fresh = feed(handle(1, fs, ch), [b])[0][0]
    cont = handle(1, fs, ch)
    feed(cont, [a])
    goes_on = feed(cont, [b])[0][0]
    assert len(fresh) == 2 and len(goes_on) > 2

    def primed(n=2):
        dec = handle(n, fs, ch)
        feed(dec, [a] * n)
        return dec

    def expect(dec, restarted):
        got, _, _ = feed(dec, [b] * len(restarted))
        for s, r in enumerate(restarted):
            assert same(got[s], fresh if r else goes_on), (s, r)

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
    tail, oc, _ = feed(dec, [a[:0], a[:7]], flush=True)  # its own flush restarts both
    assert list(oc) == [-(-len(a) // H) - 2, -(-(len(a) + 7) // H) - 2]
    expect(dec, [True, True])
    dec = primed()
    dec.set_pitch(True, 60, 500, 154 / 1024.0)
    expect(dec, [True, True])
    dec = primed()
    dec.set_output(fs, ch)  # turns the sink off
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.pitch(np.ascontiguousarray(a[None]), [len(a)])
    dec.set_pitch(True, 60, 500, 154 / 1024.0)
    expect(dec, [True, True])
    dec = primed()
    dec.set_pitch(False)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.pitch(np.ascontiguousarray(a[None]), [len(a)])
    # the other sinks' states are not this one's: a segment call in between changes nothing
    dec = primed()
    dec.set_segments(True)
    dec.segments(np.ascontiguousarray(a[None]), [len(a)])
    expect(dec, [False, False])


@pytest.fixture(scope="module")
def batch():
    return Batch()


def test_argument_errors(batch):
    fs, ch = 48000, 2
    L = mp3_amd.lib()
    x = np.ascontiguousarray(stereo(harmonic(fs, 150.0, 5000), ch)[None])
    dec = mp3_amd.BatchDecoder(2, 1)
    assert L.mp3d_batch_set_pitch(dec._h, 1, 60, 500, 154) == -1  # no packed format yet
    dec.set_output(fs, ch)
    cnt, oc = np.array([5000, 0], np.int32), np.zeros(2, np.int32)
    rec = np.zeros((2, 16), DT)

    def call(flags=0, n=1, sp=x.ctypes.data, gp=rec.ctypes.data, cp=cnt.ctypes.data, scp=oc.ctypes.data, stride=5000,
             gstride=16):
        return L.mp3d_batch_pitch(dec._h, sp, stride, cp, n, gp, gstride, scp, flags, None)

    assert call() == -1  # before set_pitch
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.pitch(x, [5000])
    offs, sizes = batch.geom(0, 1)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_pitch(batch.blob, offs[:2], sizes[:2], 1)
    for bad in [(49, 500, 154), (60, 60, 154), (500, 60, 154), (60, 2001, 154), (60, 500, 0), (60, 500, 1025),
                (60, 500, -1)]:
        assert L.mp3d_batch_set_pitch(dec._h, 1, *bad) == -1, bad
    assert call() == -1  # refused parameters leave the sink off
    assert L.mp3d_batch_set_pitch(dec._h, 1, 50, 2000, 1024) == 0 and L.mp3d_batch_set_pitch(dec._h, 1, 1999, 2000, 1) == 0
    low = mp3_amd.BatchDecoder(1, 1)
    low.set_output(8000, 1)
    assert L.mp3d_batch_set_pitch(low._h, 1, 60, 2001, 154) == -1 and L.mp3d_batch_set_pitch(low._h, 1, 60, 2000, 154) == 0
    low.set_output(11025, 1)
    assert L.mp3d_batch_set_pitch(low._h, 1, 60, 2757, 154) == -1  # 4 fmax > fs
    dec.set_pitch(True)
    assert dec._pitch == 60
    assert call(4) == -1 and call(mp3_amd.PACK_GAPLESS) == -1  # unknown flag; the stage has no frames to read a tag from
    assert call(n=3) == -5 and call(n=0) == -1
    assert call(sp=None) == -1 and call(gp=None) == -1 and call(cp=None) == -1 and call(scp=None) == -1
    assert call(stride=-1) == -1 and call(gstride=-1) == -1 and call(stride=2 ** 31 - 1) == -1 and call(gstride=2 ** 31) == -1
    dsmp = torch.zeros(2 * 5000 * ch + 4, dtype=torch.float32, device="cuda")
    drec = torch.zeros(2 * 16 * 4 + 4, dtype=torch.int32, device="cuda")
    dcnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert call(sp=dsmp.data_ptr() + 2) == -1  # misaligned device pointers
    assert call(gp=drec.data_ptr() + 4) == -1  # a device pitch is aligned to 8 bytes
    assert call(scp=dcnt.data_ptr() + 2) == -1 and call(cp=dcnt.data_ptr() + 1) == -1
    assert call(sp=dsmp.data_ptr() + 4, gp=drec.data_ptr() + 8, scp=dcnt.data_ptr() + 4) == 0
    assert call(mp3_amd.PACK_FLUSH) == 0
    dec.sync()
    # a launch too large: 2^31 - 1 - 960 samples a stream are (2^31 + ...) / H / TILE tiles, times 256 threads
    big = mp3_amd.BatchDecoder(4096, 1)
    big.set_output(8000, 1)
    big.set_pitch(True)
    bc, bo = np.zeros(4096, np.int32), np.zeros(4096, np.int32)
    brec = np.zeros((4096, 1), DT)
    assert L.mp3d_batch_pitch(big._h, dsmp.data_ptr(), 2 ** 31 - 1 - 960, bc.ctypes.data, 4096, brec.ctypes.data, 1,
                              bo.ctypes.data, 0, None) == -5

    def decode(flags=0, n=2, F=1, gp=rec.ctypes.data, scp=oc.ctypes.data):
        return L.mp3d_batch_decode_pitch(dec._h, batch.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, n, F,
                                         gp, 16, scp, flags, None, None)

    assert decode(4) == -1 and decode(gp=None) == -1 and decode(scp=None) == -1 and decode(n=3) == -5
    assert decode(F=2) == -5 and decode(n=0) == -1
    assert decode(mp3_amd.PACK_FLUSH | mp3_amd.PACK_GAPLESS) == 0
    with pytest.raises(mp3_amd.MP3DError, match="set_pitch"):
        mp3_amd.BatchDecoder(1, 1).long_pitch(b"")


@pytest.mark.parametrize("fs,ch,pi", [(48000, 2, 0), (8000, 1, 1)])
def test_host_and_device_buffers_agree(fs, ch, pi):
    fmin, fmax, theta = params(fs)[pi]
    b = batch_of(fs, ch, fmin, fmax)
    n, ss = len(b), max(1, max(len(x) for _, x in b))
    smp = torch.zeros((n, ss, ch), dtype=torch.float32, device="cuda")
    for s, (_, x) in enumerate(b):
        smp[s, : len(x)] = torch.from_numpy(x.copy()).cuda()
    hsmp = smp.cpu().numpy()
    lens = [len(x) for _, x in b]
    stride = mp3_amd.pitch_max_frames(fs, ss, fmin)
    strm = torch.cuda.Stream()
    for flush in (True, False):
        want, wc = case(fs, ch, fmin, fmax, theta)[flush]  # host in, host out
        with torch.cuda.stream(strm):
            cnt = torch.tensor(lens, dtype=torch.int32, device="cuda")
            out = torch.full((n, stride, 4), -1, dtype=torch.int32, device="cuda")
            got = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dec = handle(n, fs, ch, fmin, fmax, theta)
            dec.pitch(smp, cnt, out=out, out_counts=got, flush=flush, stream=strm.cuda_stream)  # device, device
        strm.synchronize()
        out, got = out.cpu().numpy().view(DT).reshape(n, stride), got.cpu().numpy()
        mixed, mc = handle(n, fs, ch, fmin, fmax, theta).pitch(smp, cnt, flush=flush)  # device in, host out
        dout = torch.full((n, stride, 4), -1, dtype=torch.int32, device="cuda")
        dgot = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        handle(n, fs, ch, fmin, fmax, theta).pitch(hsmp, lens, out=dout, out_counts=dgot, flush=flush)  # host, device
        torch.cuda.synchronize()
        dout, dgot = dout.cpu().numpy().view(DT).reshape(n, stride), dgot.cpu().numpy()
        for s in range(n):
            assert got[s] == wc[s] == mc[s] == dgot[s], (s, flush)
            assert same(out[s, : got[s]], want[s]) and same(mixed[s, : got[s]], want[s]), (s, flush)
            assert same(dout[s, : got[s]], want[s]) and (out[s, got[s]:].view(np.int32) == -1).all(), (s, flush)


# ---- composition ------------------------------------------------------------------
@pytest.mark.parametrize("gapless", [False, True])
def test_decode_pitch_is_the_stage_on_the_packed_samples(batch, gapless):
    fs, ch = 16000, 1
    offs, sizes = batch.geom(0, FS)
    pk = mp3_amd.BatchDecoder(batch.n, FS)
    pk.set_output(fs, ch)
    dout = torch.zeros((batch.n, mp3_amd.packed_max_samples(fs, FS), ch), dtype=torch.float32, device="cuda")
    dcnt = torch.zeros(batch.n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pk.decode_packed(batch.blob, offs, sizes, FS, out=dout, counts=dcnt, flush=True, gapless=gapless)
    pk.sync()
    smp, counts = dout.cpu().numpy(), dcnt.cpu().numpy()
    via, vc = handle(batch.n, fs, ch).pitch(dout, dcnt, flush=True)  # on the device output
    assert vc[batch.names.index("empty")] == 0 and (vc > 1).any()
    for chunks in ((FS,), (5, 11)):
        dec = handle(batch.n, fs, ch, F=max(chunks))
        got, a = [[] for _ in range(batch.n)], 0
        for i, c in enumerate(chunks):
            o, z = batch.geom(a, a + c)
            rec, oc, _ = dec.decode_pitch(batch.blob, o, z, c, flush=i == len(chunks) - 1, gapless=gapless)
            for s in range(batch.n):
                assert oc[s] >= 0
                got[s].append(rec[s, : oc[s]])
            a += c
        for s in range(batch.n):
            assert same(np.concatenate(got[s]), via[s, : vc[s]].copy()), (batch.names[s], chunks)
    for s in range(0, batch.n, 3):  # and the definition itself, on decoded audio
        differing(via[s, : vc[s]], pitch_ref(quantise(smp[s, : counts[s]]), fs, 60, 500, 154, True), batch.names[s])


def test_pitch_time(batch):
    dec = handle(batch.n, 48000, 2, F=FS)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.pitch_time_us()  # no pitch call yet
    offs, sizes = batch.geom(0, FS)
    dec.decode_pitch(batch.blob, offs, sizes, FS, flush=True)
    assert dec.pitch_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- poison -----------------------------------------------------------------------
def assert_same_case(*args):
    got, want = run_case(*args), case(*args)
    for key in want:
        assert all(same(g, w) for g, w in zip(got[key][0], want[key][0])), key
        assert np.array_equal(got[key][1], want[key][1]), key


def test_poison(monkeypatch):
    args = (48000, 2) + params(48000)[1]
    case(*args)  # (the product library's, without the poison)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    assert_same_case(*args)


def test_workgroup_lds_poison_build(monkeypatch):
    args = (22050, 1) + params(22050)[0]
    case(*args)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        assert_same_case(*args)
