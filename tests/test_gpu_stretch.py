"""GPU: the tempo sink (BatchDecoder.set_stretch / set_tempo / stretch /
decode_stretched; include/mp3d.h "tempo sink").

Reference: the header's definition in numpy (tests/test_stretch_host.py
stretch_ref: float32 for m, q and y, int64 for d; the emit rule e_of /
blocks_seen).  Every operation of the definition is exact integer arithmetic or
one float32 rounding, so every comparison here is on bits and on exact counts;
there is no tolerance.  One batch per format holds every tempo at every length
with the signal classes in turn, plus every class at every tempo at the longest
length, each stream at its own tempo; its reference is computed once.
"""
import numpy as np
import pytest
import torch

import mp3_amd
from mp3_amd import _build
from test_gpu_features import FS, Batch, check_linear
from test_gpu_loudness import Tagged
from test_stretch_host import blocks_seen, e_of, hop, out_len, periodic, stretch_ref

pytestmark = pytest.mark.gpu

FORMATS = [(48000, 2), (44100, 2), (11025, 1), (8000, 1)]
TEMPOS = [(1, 1), (1, 2), (2, 1), (9, 10), (11, 10), (3, 4), (7, 4), (999, 1000)]
CLASSES = ["noise", "silence", "dc", "periodic", "square", "harmonics"]
PATTERN = np.float32(-777.25)


def lens(fs):
    H, D = hop(fs), hop(fs) // 2
    return [0, 1, H - 1, H, H + D, 2 * H + D - 1, 2 * H + D, 2 * H + D + 1, 7 * H + 3, 23 * H + 5]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- signals and reference -------------------------------------------------------
def signals(fs, ch, n):
    """{class: float32 [n, ch]}: the second channel differs from the first."""
    H = hop(fs)
    rng = np.random.default_rng(4070 + fs + ch)
    t = np.arange(n)
    noise = rng.uniform(-1.0, 1.0, (n, ch)).astype(np.float32)
    silence = np.zeros((n, ch), np.float32)
    dc = np.full((n, ch), 0.9, np.float32)
    # +-1.0 with half-period H: the largest d, and q clamps at +-1023 (the second channel too: 0.99975 * 1024 + 0.5)
    square = np.repeat(np.where((t // H) % 2 == 0, 1.0, -1.0)[:, None], ch, 1).astype(np.float32)
    harm = np.stack([sum(0.5 / h * np.sin(2.0 * np.pi * 220.0 * h * t / fs + 0.9 * c * h) for h in (1, 2, 3))
                     for c in range(ch)], 1).astype(np.float32)
    if ch == 2:
        dc[:, 1] = -0.45
        square[:, 1] *= np.float32(0.9995)
    return {"noise": noise, "silence": silence, "dc": dc, "periodic": periodic(fs, ch, n)[0], "square": square,
            "harmonics": harm}


_sig, _case, _ref = {}, {}, {}


def sig(fs, ch):
    if (fs, ch) not in _sig:
        _sig[(fs, ch)] = signals(fs, ch, lens(fs)[-1])
    return _sig[(fs, ch)]


def streams(fs, ch):
    """[(class, length, (num, den))] of the format's batch"""
    L = lens(fs)
    out = [(CLASSES[(ti + li) % len(CLASSES)], n, tp) for ti, tp in enumerate(TEMPOS) for li, n in enumerate(L)]
    out += [(c, L[-1], tp) for tp in TEMPOS for c in CLASSES if (c, L[-1], tp) not in out]
    return out


def ref(fs, ch, name, n, tempo):
    """stretch_ref of the class's first n samples: computed once, never changed."""
    key = (fs, ch, name, n, tempo)
    if key not in _ref:
        y = stretch_ref(sig(fs, ch)[name][:n], fs, *tempo)[0]
        y.setflags(write=False)
        _ref[key] = y
    return _ref[key]


# ---- the stage -------------------------------------------------------------------
def handle(n, fs, ch, tempos=None, F=1):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(fs, ch)
    dec.set_stretch(True)
    if tempos is not None:
        dec.set_tempo([t[0] for t in tempos], [t[1] for t in tempos])
    return dec


def feed(dec, xs, flush=False, stride=None):
    """Feed xs[s] ([k, ch]) to stream s in one call; returns ([output of s], counts, raw out)."""
    n, (fs, ch) = len(xs), dec._out
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss, ch), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    cnt = np.array([len(x) for x in xs], np.int32)
    stride = stride if stride is not None else mp3_amd.stretch_max_samples(fs, ss, 1, 2)
    out = np.full((n, stride, ch), PATTERN, np.float32)
    out, oc = dec.stretch(smp, cnt, out=out, flush=flush)
    for s in range(n):
        assert (out[s, max(int(oc[s]), 0):] == PATTERN).all(), s  # nothing past the count is touched
    return [out[s, : max(int(oc[s]), 0)].copy() for s in range(n)], oc, out


def run_case(fs, ch):
    """(outputs flushed, counts flushed, outputs not flushed, counts not flushed) of the format's batch"""
    st = streams(fs, ch)
    xs = [sig(fs, ch)[c][:n] for c, n, _ in st]
    tempos = [tp for _, _, tp in st]
    a, ac, _ = feed(handle(len(st), fs, ch, tempos), xs, flush=True)
    b, bc, _ = feed(handle(len(st), fs, ch, tempos), xs)
    return a, ac, b, bc


def case(fs, ch):
    if (fs, ch) not in _case:
        _case[(fs, ch)] = run_case(fs, ch)
    return _case[(fs, ch)]


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_values(fs, ch):
    """Flushed: every stream of the batch, each at its own tempo, equals the reference bit for bit."""
    flushed, fc, _, _ = case(fs, ch)
    for s, (name, n, tempo) in enumerate(streams(fs, ch)):
        what = "%d Hz x %d, %s, %d samples at %d/%d" % ((fs, ch, name, n) + tempo)
        assert fc[s] == out_len(n, *tempo), what
        assert same_bits(flushed[s], ref(fs, ch, name, n, tempo)), what
        if tempo[0] == tempo[1]:
            assert same_bits(flushed[s], sig(fs, ch)[name][:n]), what  # y == x


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_unflushed_counts_and_prefix(fs, ch):
    _, _, open_, oc = case(fs, ch)
    H = hop(fs)
    for s, (name, n, tempo) in enumerate(streams(fs, ch)):
        what = "%d Hz x %d, %s, %d samples at %d/%d" % ((fs, ch, name, n) + tempo)
        assert oc[s] == blocks_seen(n, H, *tempo) * H, what
        assert same_bits(open_[s], ref(fs, ch, name, n, tempo)[: oc[s]]), what


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_split_invariance(fs, ch):
    """One stream per tempo, in calls cut at random points and on both sides of an emit threshold."""
    H = hop(fs)
    name, n = "noise", lens(fs)[-1]
    x = sig(fs, ch)[name][:n]
    tempos = [(1, 2), (2, 1), (9, 10), (7, 4), (1, 1)]
    rng = np.random.default_rng(99 + fs)
    cuts = []
    for num, den in tempos:
        e = e_of(5, H, num, den)
        assert e + 2 < n
        c = set(int(v) for v in rng.integers(1, n, 4)) | {e, e + 1, e + 2}  # N - 1 = e_k - 1, e_k, e_k + 1
        c = [0] + sorted(c)
        cuts.append(c + [n] * (9 - len(c)) + [n])  # (equally many calls; the last one feeds nothing and flushes)
    dec = handle(len(tempos), fs, ch, tempos)
    got = [[] for _ in tempos]
    for i in range(len(cuts[0]) - 1):
        last = i == len(cuts[0]) - 2
        outs, oc, _ = feed(dec, [x[c[i]:c[i + 1]] for c in cuts], flush=last)
        for s, (num, den) in enumerate(tempos):
            before = blocks_seen(cuts[s][i], H, num, den) * H
            want = out_len(n, num, den) - before if last else blocks_seen(cuts[s][i + 1], H, num, den) * H - before
            assert oc[s] == want, (tempos[s], i)
            got[s].append(outs[s])
    for s, tempo in enumerate(tempos):
        assert same_bits(np.concatenate(got[s]), ref(fs, ch, name, n, tempo)), tempo


def test_one_long_stream():
    """About 200 blocks at n_streams = 1: the chain of one stream alone."""
    fs, ch, tempo = 8000, 1, (1, 2)
    H = hop(fs)
    n = 100 * H + 7
    t = np.arange(n)
    x = (0.6 * np.sin(2.0 * np.pi * 220.0 * t / fs) + 0.2 * np.sin(2.0 * np.pi * 1230.0 * t / fs))[:, None]
    x = x.astype(np.float32)
    outs, oc, _ = feed(handle(1, fs, ch, [tempo]), [x], flush=True)
    assert oc[0] == 2 * n and -(-oc[0] // H) >= 200
    assert same_bits(outs[0], stretch_ref(x, fs, *tempo)[0])


# ---- decode_stretched against the stage ------------------------------------------------
DEC_FMT = (48000, 2)


def batch_tempos(n):
    return [TEMPOS[s % len(TEMPOS)] for s in range(n)]


@pytest.fixture(scope="module")
def batch():
    return Batch()


def packed_on_device(batch, gapless=False):
    fs, ch = DEC_FMT
    dec = mp3_amd.BatchDecoder(batch.n, FS)
    dec.set_output(fs, ch)
    offs, sizes = batch.geom(0, FS)
    out = torch.zeros((batch.n, mp3_amd.packed_max_samples(fs, FS), ch), dtype=torch.float32, device="cuda")
    counts = torch.zeros(batch.n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_packed(batch.blob, offs, sizes, FS, out=out, counts=counts, flush=True, gapless=gapless)
    dec.sync()
    return out, counts


def stage_on_device(batch, smp, counts):
    """The stage on decode_packed's device output, flushed: ([output of s], counts)."""
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, batch_tempos(batch.n))
    stride = mp3_amd.stretch_max_samples(fs, smp.shape[1], 1, 2)
    out = torch.full((batch.n, stride, ch), float(PATTERN), dtype=torch.float32, device="cuda")
    oc = torch.zeros(batch.n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.stretch(smp, counts, out=out, out_counts=oc, flush=True)
    dec.sync()
    out, oc = out.cpu().numpy(), oc.cpu().numpy()
    for s in range(batch.n):
        assert oc[s] >= 0 and (out[s, oc[s]:] == PATTERN).all()
    return [out[s, : oc[s]].copy() for s in range(batch.n)], oc


def decode_chunks(batch, chunks=(FS,), gapless=False):
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, batch_tempos(batch.n), F=max(chunks))
    got, a = [[] for _ in range(batch.n)], 0
    for i, c in enumerate(chunks):
        offs, sizes = batch.geom(a, a + c)
        stride = mp3_amd.stretch_max_samples(fs, mp3_amd.packed_max_samples(fs, c), 1, 2)
        out = np.full((batch.n, stride, ch), PATTERN, np.float32)
        out, oc, _ = dec.decode_stretched(batch.blob, offs, sizes, c, out=out, flush=i == len(chunks) - 1,
                                          gapless=gapless)
        for s in range(batch.n):
            assert oc[s] >= 0 and (out[s, oc[s]:] == PATTERN).all()
            got[s].append(out[s, : oc[s]].copy())
        a += c
    return [np.concatenate(g) for g in got]


@pytest.fixture(scope="module")
def decoded(batch):
    return decode_chunks(batch)


def test_decode_stretched_is_the_stage_on_the_packed_samples(batch, decoded):
    fs, ch = DEC_FMT
    smp, counts = packed_on_device(batch)
    via, oc = stage_on_device(batch, smp, counts)
    smp, counts = smp.cpu().numpy(), counts.cpu().numpy()
    assert oc[batch.names.index("empty")] == 0
    for s, tempo in enumerate(batch_tempos(batch.n)):
        assert oc[s] == out_len(int(counts[s]), *tempo), batch.names[s]
        assert same_bits(decoded[s], via[s]), batch.names[s]
    for s in (0, 1, 2):  # and the definition itself, on decoded audio
        assert same_bits(via[s], stretch_ref(smp[s, : counts[s]], fs, *batch_tempos(batch.n)[s])[0]), batch.names[s]


@pytest.mark.parametrize("chunks", [(1,) * FS, (3,) * 5 + (1,)])
def test_decode_stretched_chunking_is_bit_identical(batch, decoded, chunks):
    got = decode_chunks(batch, chunks)
    for s in range(batch.n):
        assert same_bits(got[s], decoded[s]), batch.names[s]


def test_decode_stretched_gapless(batch):
    tagged = Tagged(batch)
    smp, counts = packed_on_device(tagged, gapless=True)
    _, plain = packed_on_device(tagged)
    assert (counts.cpu().numpy() < plain.cpu().numpy()).any()  # some stream has a LAME tag: its window trims it
    via, oc = stage_on_device(tagged, smp, counts)
    got = decode_chunks(tagged, (5, 11), gapless=True)
    for s in range(tagged.n):
        assert same_bits(got[s], via[s]), tagged.names[s]


def test_stretched_samples_feed_the_feature_sink():
    """stretch's device out and counts into features(): the log-mel frames of the host-stretched reference, within
    the feature sink's own bound (test_gpu_features.check_linear)."""
    fs, ch, n_mels = 16000, 1, 80
    n = 30 * hop(fs) + 11
    t = np.arange(n)
    rng = np.random.default_rng(5)
    xs = [(0.4 * np.sin(2.0 * np.pi * 440.0 * t / fs) + 0.05 * rng.standard_normal(n)).astype(np.float32)[:, None]
          for _ in range(3)]
    tempos = [(9, 10), (1, 1), (11, 10)]
    dec = handle(3, fs, ch, tempos)
    dec.set_features(n_mels, log10=False)  # (the mel energies: check_linear's bound is for them)
    smp = torch.from_numpy(np.stack(xs)).cuda()
    cnt = torch.full((3,), n, dtype=torch.int32, device="cuda")
    stride = mp3_amd.stretch_max_samples(fs, n, 1, 2)
    out = torch.zeros((3, stride, ch), dtype=torch.float32, device="cuda")
    oc = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.stretch(smp, cnt, out=out, out_counts=oc, flush=True)
    feat, fc = dec.features(out[:, :, 0], oc, flush=True)
    dec.sync()
    for s, tempo in enumerate(tempos):
        y = stretch_ref(xs[s], fs, *tempo)[0][:, 0]
        assert fc[s] == -(-len(y) // 160)
        check_linear(feat[s, : fc[s]], y, n_mels, "stretched %d/%d" % tempo)


# ---- lifecycle -------------------------------------------------------------------
def test_restarts():
    """Every restart of the definition: the slot then answers as a fresh one does, and the others go on."""
    fs, ch = 11025, 1
    H = hop(fs)
    x = sig(fs, ch)["noise"]
    a, b = 5 * H + 3, 9 * H + 1
    tempo = (3, 4)
    fresh, fc, _ = feed(handle(1, fs, ch, [tempo]), [x[a:a + b]])
    cont = handle(1, fs, ch, [tempo])
    feed(cont, [x[:a]])
    goes_on, gc, _ = feed(cont, [x[a:a + b]])
    assert not same_bits(goes_on[0], fresh[0])

    def primed(n=2):
        dec = handle(n, fs, ch, [tempo] * n)
        feed(dec, [x[:a]] * n)
        return dec

    def expect(dec, restarted):
        outs, oc, _ = feed(dec, [x[a:a + b]] * len(restarted))
        for s, r in enumerate(restarted):
            want = fresh[0] if r else goes_on[0]
            assert same_bits(outs[s], want), (s, r)

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
    dec.set_tempo(tempo[0], tempo[1], first=1)  # a sub-range: slot 0 is left alone
    expect(dec, [False, True])
    dec = primed()
    dec.set_stretch(True)  # restarts every slot, and every tempo is 1/1 again
    outs, oc, _ = feed(dec, [x[a:a + b]] * 2, flush=True)
    assert same_bits(outs[0], x[a:a + b]) and same_bits(outs[1], x[a:a + b])
    dec = primed()
    dec.set_output(fs, ch)  # turns stretch off
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        feed(dec, [x[:a]] * 2)
    dec.set_stretch(True)
    dec.set_tempo([tempo[0]] * 2, [tempo[1]] * 2)
    expect(dec, [True, True])
    dec = primed()
    feed(dec, [x[:0], x[:7]], flush=True)  # its own flush restarts both
    expect(dec, [True, True])


def test_stride_overflow():
    fs, ch = 44100, 2
    H = hop(fs)
    x = sig(fs, ch)["noise"]
    a, b = 6 * H + 7, 4 * H
    tempo = (9, 10)
    need = blocks_seen(a, H, *tempo) * H
    assert need >= 2 * H
    dec = handle(3, fs, ch, [tempo] * 3)
    outs, oc, raw = feed(dec, [x[:a], x[:H], x[:a]], stride=need - 1)
    assert list(oc) == [-1, 0, -1]
    assert (raw == PATTERN).all()  # nothing written
    fresh, _, _ = feed(handle(1, fs, ch, [tempo]), [x[a:a + b]])
    cont = handle(1, fs, ch, [tempo])
    feed(cont, [x[:H]])
    second, _, _ = feed(cont, [x[a:a + b]])
    nxt, nc, _ = feed(dec, [x[a:a + b]] * 3)
    assert same_bits(nxt[0], fresh[0]) and same_bits(nxt[2], fresh[0])  # the two were restarted
    assert same_bits(nxt[1], second[0]) and not same_bits(second[0], fresh[0])  # the stream within the stride goes on
    outs, oc, _ = feed(handle(1, fs, ch, [tempo]), [x[:a]], stride=need)  # exactly the need fits
    assert list(oc) == [need]
    outs, oc, _ = feed(handle(1, fs, ch, [tempo]), [x[:a]], stride=a - 1, flush=True)
    assert list(oc) == [-1]


def test_argument_errors(batch):
    fs, ch = 48000, 2
    L = mp3_amd.lib()
    x = np.ascontiguousarray(sig(fs, ch)["noise"][None, :5000])
    dec = mp3_amd.BatchDecoder(2, 1)
    assert L.mp3d_batch_set_stretch(dec._h, 1) == -1  # no packed format yet
    dec.set_output(fs, ch)
    cnt, oc = np.array([5000, 0], np.int32), np.zeros(2, np.int32)
    out = np.zeros((2, 12000, ch), np.float32)
    one = np.array([1, 1], np.int32)

    def call(flags=0, n=1, sp=x.ctypes.data, op=out.ctypes.data, cp=cnt.ctypes.data, ocp=oc.ctypes.data, stride=5000,
             ostride=12000):
        return L.mp3d_batch_stretch(dec._h, sp, stride, cp, n, op, ostride, ocp, flags, None)

    def tempo(num, den, first=0, n=1):
        nu, de = np.array([num] * n, np.int32), np.array([den] * n, np.int32)
        return L.mp3d_batch_set_tempo(dec._h, first, n, nu.ctypes.data, de.ctypes.data)

    assert call() == -1 and tempo(1, 1) == -1  # before set_stretch
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.stretch(x, [5000])
    offs, sizes = batch.geom(0, 1)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_stretched(batch.blob, offs[:2], sizes[:2], 1)
    dec.set_stretch(True)
    assert call(4) == -1 and call(mp3_amd.PACK_GAPLESS) == -1  # unknown flag; the stage has no frames to read a tag from
    assert call(n=3) == -5 and call(n=0) == -1
    assert call(sp=None) == -1 and call(op=None) == -1 and call(cp=None) == -1 and call(ocp=None) == -1
    assert call(stride=-1) == -1 and call(ostride=-1) == -1
    for num, den in [(0, 1), (1, 0), (4097, 4096), (1, 3), (3, 1), (2047, 4096), (-2, -1)]:
        assert tempo(num, den) == -1, (num, den)
    assert tempo(1, 1, first=-1) == -1 and tempo(1, 1, n=0) == -1
    assert tempo(1, 1, first=1, n=2) == -5 and tempo(1, 1, first=2) == -5
    assert L.mp3d_batch_set_tempo(dec._h, 0, 1, None, one.ctypes.data) == -1
    # a bad ratio anywhere writes nothing: slot 0 stays at 1/1
    assert L.mp3d_batch_set_tempo(dec._h, 0, 2, np.array([1, 1], np.int32).ctypes.data,
                                  np.array([2, 3], np.int32).ctypes.data) == -1
    y, yc = dec.stretch(x, [5000], flush=True)
    assert yc[0] == 5000 and same_bits(y[0, :5000], x[0])
    assert tempo(4096, 2048) == 0 and tempo(2048, 4096) == 0 and tempo(1, 1) == 0
    dsmp = torch.zeros(2 * 5000 * ch + 4, dtype=torch.float32, device="cuda")
    dout = torch.zeros(2 * 12000 * ch + 8, dtype=torch.float32, device="cuda")
    dcnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert call(sp=dsmp.data_ptr() + 2) == -1  # misaligned device pointers
    assert call(op=dout.data_ptr() + 4) == -1  # a device out is aligned to one sample frame
    assert call(ocp=dcnt.data_ptr() + 2) == -1 and call(cp=dcnt.data_ptr() + 1) == -1
    assert call(sp=dsmp.data_ptr(), op=dsmp.data_ptr(), ostride=5000) == -1  # out overlapping samples
    assert call(sp=dsmp.data_ptr(), op=dsmp.data_ptr() + 4 * 5000 * ch - 8, ostride=100) == -1
    assert call(sp=x.ctypes.data, op=x.ctypes.data, ostride=5000) == -1
    assert call(sp=dsmp.data_ptr() + 4, op=dout.data_ptr() + 8, ocp=dcnt.data_ptr() + 4) == 0
    assert call(mp3_amd.PACK_FLUSH) == 0
    dec.sync()

    def decode(flags=0, n=2, F=1, op=out.ctypes.data, ocp=oc.ctypes.data):
        return L.mp3d_batch_decode_stretched(dec._h, batch.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, n, F,
                                             op, 12000, ocp, flags, None, None)

    assert decode(4) == -1 and decode(op=None) == -1 and decode(ocp=None) == -1 and decode(n=3) == -5
    assert decode(F=2) == -5 and decode(n=0) == -1
    assert decode(mp3_amd.PACK_FLUSH | mp3_amd.PACK_GAPLESS) == 0


@pytest.mark.parametrize("fs,ch", [(48000, 2), (8000, 1)])
def test_host_and_device_buffers_agree(fs, ch):
    flushed, fc, open_, oc = case(fs, ch)
    st = streams(fs, ch)[-12:]  # a dozen of the longest streams
    base = len(streams(fs, ch)) - len(st)
    n, ss = len(st), lens(fs)[-1]
    smp = torch.zeros((n, ss, ch), dtype=torch.float32, device="cuda")
    for s, (name, k, _) in enumerate(st):
        smp[s, :k] = torch.from_numpy(sig(fs, ch)[name][:k]).cuda()
    stride = mp3_amd.stretch_max_samples(fs, ss, 1, 2)
    strm = torch.cuda.Stream()
    for flush in (True, False):
        with torch.cuda.stream(strm):
            cnt = torch.tensor([k for _, k, _ in st], dtype=torch.int32, device="cuda")
            out = torch.full((n, stride, ch), float(PATTERN), dtype=torch.float32, device="cuda")
            got = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dec = handle(n, fs, ch, [tp for _, _, tp in st])
            dec.stretch(smp, cnt, out=out, out_counts=got, flush=flush, stream=strm.cuda_stream)
        strm.synchronize()
        out, got = out.cpu().numpy(), got.cpu().numpy()
        for s in range(n):
            want = (flushed if flush else open_)[base + s]
            assert got[s] == len(want) and same_bits(out[s, : got[s]], want) and (out[s, got[s]:] == PATTERN).all()
        mixed, mc = handle(n, fs, ch, [tp for _, _, tp in st]).stretch(smp, cnt, flush=flush)  # device in, host out
        for s in range(n):
            assert mc[s] == got[s] and same_bits(mixed[s, : mc[s]], out[s, : got[s]])


def test_stretch_time(batch):
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, batch_tempos(batch.n), F=FS)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.stretch_time_us()  # no stretch call yet
    offs, sizes = batch.geom(0, FS)
    dec.decode_stretched(batch.blob, offs, sizes, FS, flush=True)
    assert dec.stretch_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- poison ----------------------------------------------------------------------
def assert_same_case(fs, ch):
    got, want = run_case(fs, ch), case(fs, ch)
    for g, w in zip(got[0] + got[2], want[0] + want[2]):
        assert same_bits(g, w)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_poison(batch, decoded, fs, ch, monkeypatch):
    case(fs, ch)  # (the product library's, without the poison)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    assert_same_case(fs, ch)
    if (fs, ch) == DEC_FMT:
        for g, w in zip(decode_chunks(batch, (5, 11)), decoded):
            assert same_bits(g, w)


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_workgroup_lds_poison_build(batch, decoded, fs, ch, monkeypatch):
    case(fs, ch)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        assert_same_case(fs, ch)
        if (fs, ch) == DEC_FMT:
            for g, w in zip(decode_chunks(batch, (5, 11)), decoded):
                assert same_bits(g, w)
