"""GPU: the log-mel feature sink (BatchDecoder.set_features / decode_features
/ features; include/mp3d.h "log-mel feature sink").

Reference: the header's definition in float64 numpy (frames of the float32
samples, periodic Hann, 400-point real FFT, power, the library's own float32
filterbank in float64).  Error bound per cell, from the header: with
A = sum_n |w[n] x[n]| over the frame and d = 408 * 2^-24 * A (400 accumulated
products plus twiddle, window and unpack roundings; no evaluation order does
worse),
    |mel_gpu - mel_ref| <= (sum_k F[j][k]) (2 sqrt 2 A d + 2 d^2) + 8 * 2^-24 mel_ref
and for the log output, against the same call's linear output,
    |out - log10(max(lin_gpu, 1e-10))| <= 4 * 2^-24 max(1, |out|).
The bound is loose; each value test prints max(err / bound) per input class
(DESIGN.md section 4d records them).  Measured on an MI355X, 80 / 128 mels:
impulses 4.2e-3 / 5.6e-3, tone 1.1e-3 / 1.4e-3, noise 9.8e-5 / 9.6e-5, decoded
streams 3.3e-3 / 3.4e-3.
"""
import numpy as np
import pytest
import torch

import _gen
import _golden
import mp3_amd
from _state import state_view
from mp3_amd import _build

pytestmark = pytest.mark.gpu

GOLD = ["c3_s0", "c5_mono_48k_crc", "c5_dual_32k_vbr", "lsf_22k_js", "lsf_8k_js", "lsf_16k_mono_crc",
        "keypress_128k_js"]
CASES = [(80, False), (80, True), (128, False), (128, True)]
PATTERN = np.float32(-777.25)
U = 2.0 ** -24


# ---- reference -----------------------------------------------------------------
def emitted(n):
    return (n - 200) // 160 + 1 if n >= 200 else 0


def ceil_frames(n):
    return -(-n // 160)


_fb = {}


def fb64(n_mels):
    if n_mels not in _fb:
        _fb[n_mels] = mp3_amd.mel_filterbank(n_mels).astype(np.float64)
    return _fb[n_mels]


def reference(x, T, n_mels):
    """(mel float64 [T, n_mels], bound [T, n_mels]) of frames 0 .. T - 1 of x."""
    x = np.asarray(x, np.float32).astype(np.float64)
    xp = np.concatenate([np.zeros(200), x, np.zeros(160 * T + 400)])
    idx = 160 * np.arange(T)[:, None] + np.arange(400)[None, :]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 400.0)
    y = xp[idx] * w[None, :]
    X = np.fft.rfft(y, axis=1)
    P = X.real ** 2 + X.imag ** 2
    F = fb64(n_mels)
    mel = P @ F.T
    A = np.abs(y).sum(axis=1)[:, None]
    d = 408.0 * U * A
    bound = F.sum(axis=1)[None, :] * (2.0 * np.sqrt(2.0) * A * d + 2.0 * d * d) + 8.0 * U * mel
    return mel, bound


def check_linear(got, x, n_mels, what):
    """got float32 [T, n_mels] against the reference; returns max(err / bound)."""
    mel, bound = reference(x, got.shape[0], n_mels)
    err = np.abs(got.astype(np.float64) - mel)
    ratio = float((err / np.maximum(bound, 1e-300)).max(initial=0.0))
    print("%s, %d mels: %d frames, max err/bound %.3g" % (what, n_mels, got.shape[0], ratio))
    assert (err <= bound).all(), (what, ratio)
    return ratio


def check_log(got_log, got_lin, what):
    want = np.log10(np.maximum(got_lin.astype(np.float64), 1e-10))
    err = np.abs(got_log.astype(np.float64) - want)
    tol = 4.0 * U * np.maximum(1.0, np.abs(got_log.astype(np.float64)))
    assert (err <= tol).all(), (what, float((err / tol).max(initial=0.0)))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the tap -------------------------------------------------------------------
def handle(n, n_mels, log, F=1):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(16000, 1)
    dec.set_features(n_mels, log10=log)
    return dec


def tap(dec, xs, flush=False, stride=None):
    """Feed xs[s] to stream s; returns ([frames of s], counts, raw feat)."""
    n = len(xs)
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    cnt = np.array([len(x) for x in xs], np.int32)
    stride = stride if stride is not None else (ss + 200 + 159) // 160 + 1
    feat = np.full((n, stride, dec._mels), PATTERN, np.float32)
    feat, fc = dec.features(smp, cnt, feat=feat, flush=flush)
    for s in range(n):
        assert (feat[s, max(int(fc[s]), 0):] == PATTERN).all(), s  # nothing past the frames is touched
    return [feat[s, : max(int(fc[s]), 0)].copy() for s in range(n)], fc, feat


def signals():
    n = 4800
    imp = np.zeros(n, np.float32)
    imp[[0, 199, 200, 359, 1000]] = 1.0
    tone = (0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / 16000.0)).astype(np.float32)
    noise = (np.random.default_rng(1234).standard_normal(n) * 0.25).astype(np.float32)
    return {"impulses": imp, "tone": tone, "noise": noise}


@pytest.fixture(scope="module")
def lin_tap():
    """{n_mels: linear frames of the three signals, flushed}: computed once."""
    out = {}
    sig = signals()
    for nm in (80, 128):
        frames, fc, _ = tap(handle(3, nm, False), list(sig.values()), flush=True)
        assert list(fc) == [30, 30, 30]
        out[nm] = dict(zip(sig, frames))
    return out


@pytest.mark.parametrize("n_mels,log", CASES)
def test_tap_values(lin_tap, n_mels, log):
    sig = signals()
    if not log:
        for name, x in sig.items():
            check_linear(lin_tap[n_mels][name], x, n_mels, name)
        return
    frames, fc, _ = tap(handle(3, n_mels, True), list(sig.values()), flush=True)
    assert list(fc) == [30, 30, 30]
    for name, got in zip(sig, frames):
        check_log(got, lin_tap[n_mels][name], name)


@pytest.mark.parametrize("n_mels,log", CASES)
def test_tap_counts(n_mels, log):
    noise = signals()["noise"]
    lens = [0, 199, 200, 360, 4800]
    xs = [noise[:k] for k in lens]
    frames, fc, _ = tap(handle(len(xs), n_mels, log), xs)
    assert list(fc) == [emitted(k) for k in lens] == [0, 0, 1, 2, 29]
    dec = handle(len(xs), n_mels, log)
    flushed, fc2, _ = tap(dec, xs, flush=True)
    assert list(fc2) == [ceil_frames(k) for k in lens] == [0, 2, 2, 3, 30]
    for s in range(len(xs)):  # the frames emitted without the flush are the flushed run's first
        assert same_bits(frames[s], flushed[s][: fc[s]]), s
    # a flush with nothing new emits the rest, then the streams are restarted
    dec = handle(len(xs), n_mels, log)
    tap(dec, xs)
    rest, fc3, _ = tap(dec, [noise[:0]] * len(xs), flush=True)
    assert list(fc3) == [ceil_frames(k) - emitted(k) for k in lens]
    for s in range(len(xs)):
        assert same_bits(rest[s], flushed[s][fc[s]:]), s
    again, fc4, _ = tap(dec, xs, flush=True)
    assert list(fc4) == list(fc2) and all(same_bits(a, b) for a, b in zip(again, flushed))


@pytest.mark.parametrize("n_mels,log", CASES)
def test_split_invariance(n_mels, log):
    x = signals()["noise"]
    whole, _, _ = tap(handle(1, n_mels, log), [x], flush=True)

    def pieces(sizes):
        dec = handle(1, n_mels, log)
        got, a = [], 0
        for k in sizes:
            got.append(tap(dec, [x[a:a + k]])[0][0])
            a += k
        got.append(tap(dec, [x[a:]], flush=True)[0][0])
        total = np.concatenate(got)
        return total

    assert whole[0].shape[0] == 30
    assert same_bits(pieces([1, 159, 160, 161, 400]), whole[0])
    assert same_bits(pieces([1] * 400), whole[0])


# ---- decode_features against the tap -------------------------------------------
class Batch:
    """The ragged batch of tests/test_gpu_packed.py: seven goldens, the empty
    stream, a 5 x 7 C5 batch; 16 frame slots."""

    def __init__(self):
        streams = [_golden.case(nm)[0] for nm in GOLD] + [b""]
        buf, offs, sizes = _gen.batch(_gen.C5, 4242, 5, 7)
        streams += [bytes(buf[offs[s]:offs[s] + sizes[s]]) for s in range(5)]
        self.names = GOLD + ["empty"] + ["c5_%d" % s for s in range(5)]
        self.streams = streams
        self.n = len(streams)
        self.slots = [mp3_amd.long_plan(d)[0].astype(np.int64) if d else np.zeros(0, np.int64) for d in streams]
        self.F = max(len(s) for s in self.slots)
        self.base = np.concatenate([[0], np.cumsum([len(d) for d in streams])[:-1]]).astype(np.int64)
        self.blob = np.frombuffer(b"".join(streams) + b"\0" * 64, np.uint8)

    def geom(self, a=0, b=None):
        offs, sizes = [], []
        for s, d in enumerate(self.streams):
            sl = self.slots[s]
            lo = 0 if a == 0 else (int(sl[a]) if a < len(sl) else len(d))
            hi = len(d) if b is None or b >= len(sl) else int(sl[b])
            offs.append(self.base[s] + lo)
            sizes.append(hi - lo)
        return np.array(offs, np.uint64), np.array(sizes, np.uint32)


@pytest.fixture(scope="module")
def batch():
    return Batch()


FS = 16  # frame slots decoded (the longest golden has more)


@pytest.fixture(scope="module")
def packed(batch):
    """decode_packed(flush) of a fresh handle: samples, counts, infos, state."""
    dec = mp3_amd.BatchDecoder(batch.n, FS)
    dec.set_output(16000, 1)
    offs, sizes = batch.geom(0, FS)
    out, counts, infos = dec.decode_packed(batch.blob, offs, sizes, FS, flush=True)
    return out[:, :, 0].copy(), counts, infos, dec.get_state()


def decode_chunks(batch, n_mels, log, chunks=(FS,)):
    """decode_features over frame slots in calls of the given sizes, flush on
    the last: ([frames of s], total counts, infos of all slots, state)."""
    dec = handle(batch.n, n_mels, log, F=max(chunks))
    got, infos, a = [[] for _ in range(batch.n)], [], 0
    for i, c in enumerate(chunks):
        offs, sizes = batch.geom(a, a + c)
        feat = np.full((batch.n, mp3_amd.feat_max_frames(c), n_mels), PATTERN, np.float32)
        feat, fc, inf = dec.decode_features(batch.blob, offs, sizes, c, feat=feat, flush=i == len(chunks) - 1)
        for s in range(batch.n):
            assert fc[s] >= 0 and (feat[s, fc[s]:] == PATTERN).all()
            got[s].append(feat[s, : fc[s]].copy())
        infos.append(inf)
        a += c
    frames = [np.concatenate(g) for g in got]
    return frames, np.array([f.shape[0] for f in frames]), np.concatenate(infos, axis=1), dec.get_state()


@pytest.fixture(scope="module")
def decoded(batch):
    """{(n_mels, log): decode_features(flush) in one call}: computed once."""
    return {c: decode_chunks(batch, *c) for c in CASES}


@pytest.mark.parametrize("n_mels,log", CASES)
def test_decode_features_is_the_tap_on_the_packed_samples(batch, packed, decoded, n_mels, log):
    smp, counts, infos, state = packed
    frames, fc, got_infos, got_state = decoded[(n_mels, log)]
    assert np.array_equal(got_infos, infos) and np.array_equal(got_state, state)  # the same call sizes: every byte
    assert list(fc) == [ceil_frames(int(k)) for k in counts] and fc[batch.names.index("empty")] == 0
    via_tap, tc, _ = tap(handle(batch.n, n_mels, log), [smp[s, : counts[s]] for s in range(batch.n)], flush=True)
    assert np.array_equal(tc, fc)
    for s in range(batch.n):
        assert same_bits(frames[s], via_tap[s]), batch.names[s]
    if log:
        for s in range(batch.n):
            check_log(frames[s], decoded[(n_mels, False)][0][s], batch.names[s])
    else:
        worst = max(check_linear(frames[s], smp[s, : counts[s]], n_mels, batch.names[s]) for s in range(batch.n))
        print("decoded streams, %d mels: max err/bound %.3g" % (n_mels, worst))


@pytest.mark.parametrize("n_mels,log", [(80, True), (128, False)])
@pytest.mark.parametrize("chunks", [(5, 11), (1,) * 16])
def test_decode_features_chunking_is_bit_identical(batch, decoded, n_mels, log, chunks):
    frames, fc, infos, state = decoded[(n_mels, log)]
    got, gc, ginfos, gstate = decode_chunks(batch, n_mels, log, chunks)
    assert np.array_equal(gc, fc) and np.array_equal(ginfos, infos)
    assert np.array_equal(state_view(gstate), state_view(state))  # (bytes past res_len depend on the call sizes)
    for s in range(batch.n):
        assert same_bits(got[s], frames[s]), batch.names[s]


# ---- lifecycle -----------------------------------------------------------------
def test_argument_errors(batch):
    offs, sizes = batch.geom()
    x = signals()["noise"]
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    L = mp3_amd.lib()
    assert L.mp3d_batch_set_features(dec._h, 80, 1) == -1  # no packed sink yet
    dec.set_output(16000, 1)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_features(batch.blob, offs, sizes, batch.F)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.features(x[None, :], [x.size])
    for hz, ch in [(48000, 2), (16000, 2), (48000, 1)]:
        dec.set_output(hz, ch)
        assert L.mp3d_batch_set_features(dec._h, 80, 1) == -1
    dec.set_output(16000, 1)
    for nm, flags in [(129, 1), (-1, 1), (80, 2), (80, -1)]:
        assert L.mp3d_batch_set_features(dec._h, nm, flags) == -1
    dec.set_features(80)
    dec.decode_features(batch.blob, offs, sizes, batch.F, flush=True)
    dec.set_output(16000, 1)  # any later set_output turns the features off
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_features(batch.blob, offs, sizes, batch.F)
    dec.set_features(80)
    dec.set_features(0)  # off: the buffers are freed, packed calls still work
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.features(x[None, :], [x.size])
    dec.reset()
    out, counts, _ = dec.decode_packed(batch.blob, offs, sizes, batch.F, flush=True)
    assert counts.max() > 0
    # device pointers must be int-aligned: counts and feat_count as well
    dec = handle(2, 80, True)
    x5 = np.ascontiguousarray((np.random.default_rng(5).standard_normal((1, 5000)) * 0.25).astype(np.float32))
    cnt, fc = np.array([5000], np.int32), np.zeros(1, np.int32)
    feat = np.zeros((1, 40, 80), np.float32)
    dcnt = torch.tensor([0, 5000, 0, 0], dtype=torch.int32, device="cuda")
    dfc = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(cp=cnt.ctypes.data, fcp=fc.ctypes.data):
        return L.mp3d_batch_features(dec._h, x5.ctypes.data, 5000, cp, 1, feat.ctypes.data, 40, fcp, mp3_amd.PACK_FLUSH,
                                     None)

    assert call(cp=dcnt.data_ptr() + 1) == -1 and call(cp=dcnt.data_ptr() + 2) == -1
    assert call(fcp=dfc.data_ptr() + 2) == -1
    assert call() == 0 and fc[0] == ceil_frames(5000)
    assert call(cp=dcnt.data_ptr() + 4, fcp=dfc.data_ptr() + 4) == 0
    dec.sync()
    assert dfc.cpu().tolist() == [0, int(fc[0]), 0, 0]


def test_off_and_on_again(batch, decoded):
    """Each sink turned off (its buffers freed) and on again: the features
    off and on, then the output format changed and back with the features set
    again.  After each, the same flushed call on a reset decoder state gives
    the bits of a fresh handle."""
    n_mels, log = 80, True
    frames, fc, infos, _ = decoded[(n_mels, log)]
    offs, sizes = batch.geom(0, FS)
    dec = handle(batch.n, n_mels, log, F=FS)

    def call(what):
        feat = np.full((batch.n, mp3_amd.feat_max_frames(FS), n_mels), PATTERN, np.float32)
        feat, got, inf = dec.decode_features(batch.blob, offs, sizes, FS, feat=feat, flush=True)
        assert np.array_equal(got, fc) and np.array_equal(inf, infos), what
        for s in range(batch.n):
            assert same_bits(feat[s, : got[s]], frames[s]) and (feat[s, got[s]:] == PATTERN).all(), (what, s)

    call("first")
    dec.set_features(0)
    dec.reset()
    dec.set_features(n_mels, log10=log)
    call("features off and on")
    dec.set_output(48000, 2)
    dec.set_output(16000, 1)
    dec.reset()
    dec.set_features(n_mels, log10=log)
    call("another output format and back")


def test_reset_and_set_state_restart_their_slots():
    x = signals()["noise"]
    nm = 80
    cont, _, _ = tap(handle(1, nm, True), [x[:1500]])          # frames 0 .. E(1500) - 1 of x
    fresh, _, _ = tap(handle(1, nm, True), [x[500:1500]])      # x[500:] as a new stream
    assert cont[0].shape[0] == emitted(1500) and fresh[0].shape[0] == emitted(1000)
    dec = handle(3, nm, True)
    first, fc, _ = tap(dec, [x[:500]] * 3)
    assert list(fc) == [emitted(500)] * 3
    dec.set_state(mp3_amd.BatchDecoder(1, 1).get_state(0, 1), first=1)
    second, fc, _ = tap(dec, [x[500:1500]] * 3)
    for s in (0, 2):  # untouched slots go on
        assert same_bits(np.concatenate([first[s], second[s]]), cont[0]), s
    assert same_bits(second[1], fresh[0])  # the restored slot starts again
    dec.reset()
    third, _, _ = tap(dec, [x[500:1500]] * 3)
    for s in range(3):
        assert same_bits(third[s], fresh[0]), s


def test_stride_overflow():
    x = signals()["noise"]
    nm = 80
    dec = handle(3, nm, False)
    need = emitted(4800)
    frames, fc, feat = tap(dec, [x, x[:1000], x], stride=need - 1)
    assert list(fc) == [-1, emitted(1000), -1]
    assert (feat[0] == PATTERN).all() and (feat[2] == PATTERN).all()  # nothing written
    want1, _, _ = tap(handle(1, nm, False), [x[:2000]])
    fresh, _, _ = tap(handle(1, nm, False), [x[1000:2000]])
    nxt, fc, _ = tap(dec, [x[1000:2000]] * 3)
    assert same_bits(np.concatenate([frames[1], nxt[1]]), want1[0])  # the stream within the stride goes on
    assert same_bits(nxt[0], fresh[0]) and same_bits(nxt[2], fresh[0])  # the others were restarted
    # exactly the need fits
    frames, fc, _ = tap(handle(1, nm, False), [x], stride=need)
    assert list(fc) == [need]


@pytest.mark.parametrize("n_mels,log", [(80, True), (128, False)])
def test_host_and_device_buffers_agree(batch, decoded, n_mels, log):
    """Every argument a torch tensor on a caller's stream: the kernels' own
    stores land in the caller's buffer, the pattern past them stays."""
    frames, fc, infos, _ = decoded[(n_mels, log)]
    stride = mp3_amd.feat_max_frames(FS)
    dec = handle(batch.n, n_mels, log, F=FS)
    offs, sizes = batch.geom(0, FS)
    strm = torch.cuda.Stream()
    with torch.cuda.stream(strm):
        d_in = torch.from_numpy(batch.blob.copy()).cuda()
        feat = torch.full((batch.n, stride, n_mels), float(PATTERN), dtype=torch.float32, device="cuda")
        counts = torch.full((batch.n,), -7, dtype=torch.int32, device="cuda")
        d_infos = torch.zeros((batch.n, FS, 6), dtype=torch.int32, device="cuda")
        dec.decode_features(d_in, offs, sizes, FS, feat=feat, counts=counts, infos=d_infos, flush=True,
                            stream=strm.cuda_stream)
    strm.synchronize()
    feat, counts = feat.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts, fc)
    for s in range(batch.n):
        assert same_bits(feat[s, : fc[s]], frames[s]) and (feat[s, fc[s]:] == PATTERN).all(), batch.names[s]
    got_infos = d_infos.cpu().numpy().reshape(-1).view(mp3_amd.FRAME_INFO_DT).reshape(batch.n, FS)
    assert np.array_equal(got_infos, infos)
    # the tap with device samples, counts and outputs
    x = signals()["noise"]
    want, wc, _ = tap(handle(2, n_mels, log), [x, x[:777]], flush=True)
    smp = torch.zeros((2, x.size), dtype=torch.float32, device="cuda")
    smp[0] = torch.from_numpy(x).cuda()
    smp[1, :777] = torch.from_numpy(x[:777]).cuda()
    cnt = torch.tensor([x.size, 777], dtype=torch.int32, device="cuda")
    feat = torch.full((2, 32, n_mels), float(PATTERN), dtype=torch.float32, device="cuda")
    fcd = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec2 = handle(2, n_mels, log)
    dec2.features(smp, cnt, feat=feat, feat_counts=fcd, flush=True)
    dec2.sync()
    feat, fcd = feat.cpu().numpy(), fcd.cpu().numpy()
    assert np.array_equal(fcd, wc)
    for s in range(2):
        assert same_bits(feat[s, : wc[s]], want[s]) and (feat[s, wc[s]:] == PATTERN).all()


def test_feature_time(batch):
    dec = handle(batch.n, 80, True, F=batch.F)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.feature_time_us()  # no feature call yet
    offs, sizes = batch.geom()
    dec.decode_features(batch.blob, offs, sizes, batch.F, flush=True)
    assert dec.feature_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- poison --------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,log", [(80, True), (128, False)])
def test_poison(batch, decoded, n_mels, log, monkeypatch):
    frames, fc, _, _ = decoded[(n_mels, log)]
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    for chunks in ((16,), (5, 11)):
        got, gc, _, _ = decode_chunks(batch, n_mels, log, chunks)
        assert np.array_equal(gc, fc)
        for s in range(batch.n):
            assert same_bits(got[s], frames[s]), batch.names[s]


@pytest.mark.parametrize("n_mels,log", [(80, True), (128, False)])
def test_workgroup_lds_poison_build(batch, decoded, n_mels, log, monkeypatch):
    frames, fc, _, _ = decoded[(n_mels, log)]
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        got, gc, _, _ = decode_chunks(batch, n_mels, log, (5, 11))
    assert np.array_equal(gc, fc)
    for s in range(batch.n):
        assert same_bits(got[s], frames[s]), batch.names[s]
