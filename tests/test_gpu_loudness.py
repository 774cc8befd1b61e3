"""GPU: the loudness sink (BatchDecoder.set_loudness / loudness /
decode_loudness / integrated_lufs; include/mp3d.h "loudness sink").

Reference: the header's definition in float64 numpy (tests/
test_loudness_host.py: coef64, kweight64, blocks64, integrated64).  Bound per
block, from the header: with C the channel count and P the largest |x| of the
stream since its restart,
    |z_gpu - z_ref| <= 2^-22 z_ref + 1e-9 * C * P^2
(the float32 rounding of the result with a factor 4 of margin, plus double
rounding through a filter whose state gain is about 1.6e5 at 48 kHz, taken 25x
wide).  The bound is derived, not measured; each value test prints
max(err / bound) per signal class (DESIGN.md section 4e records them).
Measured on an MI355X, the largest of the four formats: unit impulse 0.051,
997 Hz sine 0.201, noise 0.157, DC step 0.117, quiet after loud 0.186, one long
stream 0.208, decoded streams 0.207: the float32 rounding of the result (half
an ulp is 0.25 of the bound).
"""
import re

import numpy as np
import pytest
import torch

import mp3_amd
from mp3_amd import _build
from test_gpu_features import FS, Batch
from test_loudness_host import block_len, blocks64, integrated64

pytestmark = pytest.mark.gpu

TILE = int(re.search(r"^#define MP3D_LD_TILE\s+(\d+)", (_build.CSRC / "mp3d_loudness.h").read_text(), re.M).group(1))
FORMATS = [(48000, 2), (44100, 2), (11025, 1), (8000, 1)]
PATTERN = np.float32(-777.25)


def nmax(fs):
    """Samples of the longest stream of the tap-values case (and of the cached signals)."""
    return max(3 * TILE + 17, 3 * block_len(fs) + 7)


# ---- signals and reference -------------------------------------------------------
def signals(fs, ch, n):
    """{class: float32 [n, ch]}: the second channel differs from the first."""
    H = block_len(fs)
    rng = np.random.default_rng(20260 + fs + ch)
    t = np.arange(n)
    imp = np.zeros((n, ch), np.float32)
    imp[0, 0] = 1.0
    sine = np.stack([0.5 * np.sin(2.0 * np.pi * 997.0 * t / fs + 0.7 * c) for c in range(ch)], 1).astype(np.float32)
    noise = rng.uniform(-1.0, 1.0, (n, ch)).astype(np.float32)
    step = np.full((n, ch), 0.9, np.float32)
    quiet = rng.uniform(-1.0, 1.0, (n, ch)).astype(np.float32)
    quiet[2 * H:] *= np.float32(1e-4)
    if ch == 2:
        imp[5, 1] = -1.0
        step[:, 1] = -0.45
    return {"impulse": imp, "sine": sine, "noise": noise, "dc step": step, "quiet after loud": quiet}


_sig, _ref = {}, {}


def sig(fs, ch, n=None):
    n = nmax(fs) if n is None else n
    if (fs, ch, n) not in _sig:
        _sig[(fs, ch, n)] = signals(fs, ch, n)
    return _sig[(fs, ch, n)]


def ref(fs, ch, name, n=None):
    n = nmax(fs) if n is None else n
    """z float64 of the whole signal: computed once, never changed."""
    if (fs, ch, name, n) not in _ref:
        z = blocks64(sig(fs, ch, n)[name], fs)
        z.setflags(write=False)
        _ref[(fs, ch, name, n)] = z
    return _ref[(fs, ch, name, n)]


def bound_of(zref, x):
    P = float(np.abs(x).max(initial=0.0))
    return 2.0 ** -22 * zref + 1e-9 * x.shape[1] * P * P


def check(got, zref, x, what, scale=1.0):
    """got float32 [k] against zref[:k] for the stream fed x; returns max(err / bound)."""
    k = got.shape[0]
    b = bound_of(zref[:k], x)
    err = np.abs(got.astype(np.float64) - zref[:k])
    ratio = float((err / b).max(initial=0.0))
    print("%s: %d blocks, max err/bound %.3g" % (what, k, ratio))
    assert (err <= scale * b).all(), (what, ratio)
    return ratio


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the tap ---------------------------------------------------------------------
def handle(n, fs, ch, F=1):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(fs, ch)
    dec.set_loudness(True)
    return dec


def tap(dec, xs, flush=False, stride=None):
    """Feed xs[s] ([k, ch]) to stream s; returns ([blocks of s], counts, peak, raw blocks)."""
    n, (fs, ch) = len(xs), dec._out
    H = block_len(fs)
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss, ch), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    cnt = np.array([len(x) for x in xs], np.int32)
    stride = stride if stride is not None else (H - 1 + ss) // H + 1
    blocks = np.full((n, stride), PATTERN, np.float32)
    blocks, bc, pk = dec.loudness(smp, cnt, blocks=blocks, flush=flush)
    for s in range(n):
        assert (blocks[s, max(int(bc[s]), 0):] == PATTERN).all(), s  # nothing past the blocks is touched
        assert pk[s] == np.abs(xs[s]).max(initial=0.0), s  # the sample peak, exact
    return [blocks[s, : max(int(bc[s]), 0)].copy() for s in range(n)], bc, pk, blocks


def tap_lengths(fs):
    H = block_len(fs)
    return [0, 1, H - 1, H, 3 * H + 7, 3 * TILE + 17]


def run_tap_case(fs, ch):
    """{class: (blocks of the six streams, counts, peak)} of one call each."""
    out = {}
    for name, x in sig(fs, ch).items():
        got, bc, pk, _ = tap(handle(6, fs, ch), [x[:k] for k in tap_lengths(fs)])
        out[name] = (got, bc, pk)
    return out


_tap = {}


def tap_case(fs, ch):
    if (fs, ch) not in _tap:
        _tap[(fs, ch)] = run_tap_case(fs, ch)
    return _tap[(fs, ch)]


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_tap_values(fs, ch):
    H = block_len(fs)
    lens = tap_lengths(fs)
    for name, (got, bc, pk) in tap_case(fs, ch).items():
        x = sig(fs, ch)[name]
        assert list(bc) == [k // H for k in lens], name
        worst = max(check(got[s], ref(fs, ch, name), x[:k], "%d Hz x %d, %s, %d samples" % (fs, ch, name, k))
                    for s, k in enumerate(lens))
        print("tap %d Hz x %d, %s: max err/bound %.3g" % (fs, ch, name, worst))


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_split_invariance(fs, ch):
    H = block_len(fs)
    sizes = [1, 7, H - 1, H + 1, TILE, TILE + 1]
    n = sum(sizes) + 2 * H + 5
    for name, x in sig(fs, ch, n).items():
        whole, wc, _, _ = tap(handle(1, fs, ch), [x])
        again, _, _, _ = tap(handle(1, fs, ch), [x])
        assert wc[0] == n // H and same_bits(whole[0], again[0]), name  # the same call: the same bits
        zref = ref(fs, ch, name, n)
        check(whole[0], zref, x, "whole, " + name)
        dec = handle(1, fs, ch)
        got, a, total = [], 0, 0
        for k in sizes + [n - sum(sizes)]:
            g, bc, _, _ = tap(dec, [x[a:a + k]])
            assert bc[0] == (a + k) // H - a // H, (name, a, k)
            got.append(g[0])
            total += int(bc[0])
            a += k
        assert total == n // H
        got = np.concatenate(got)
        err = np.abs(got.astype(np.float64) - whole[0].astype(np.float64))
        b = bound_of(zref[: n // H], x)
        print("split %d Hz x %d, %s: max |split - whole| / bound %.3g" % (fs, ch, name, float((err / b).max())))
        assert (err <= 2.0 * b).all(), name
        check(got, zref, x, "split, " + name)


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_flush(fs, ch):
    H = block_len(fs)
    x = sig(fs, ch)["noise"]
    k = H + H // 2
    fresh, fc, _, _ = tap(handle(1, fs, ch), [x[:nmax(fs)]])
    dec = handle(1, fs, ch)
    got, bc, _, _ = tap(dec, [x[:k]], flush=True)
    assert list(bc) == [1] and same_bits(got[0], fresh[0][:1])  # the partial block is dropped
    again, ac, _, _ = tap(dec, [x[:nmax(fs)]])
    assert np.array_equal(ac, fc) and same_bits(again[0], fresh[0])  # and the stream restarted
    # a flush with nothing new: nothing emitted, the open block is dropped
    dec = handle(1, fs, ch)
    tap(dec, [x[:k]])
    rest, rc, pk, _ = tap(dec, [x[:0]], flush=True)
    assert list(rc) == [0] and pk[0] == 0.0
    again, ac, _, _ = tap(dec, [x[:nmax(fs)]])
    assert same_bits(again[0], fresh[0])


@pytest.mark.parametrize("n", [200003, 66 * TILE + 1234])  # (the second: past the 64 tiles of one carry scan)
def test_one_long_stream(n):
    fs = 48000
    assert n >= 12 * TILE
    x = (np.random.default_rng(77).uniform(-0.6, 0.6, (n, 1)) + 0.3).astype(np.float32)
    got, bc, _, _ = tap(handle(1, fs, 1), [x])
    assert list(bc) == [n // block_len(fs)]
    check(got[0], blocks64(x, fs), x, "one long stream, %d tiles" % -(-n // TILE))


# ---- decode_loudness against the tap ---------------------------------------------
@pytest.fixture(scope="module")
def batch():
    return Batch()


def decode_chunks(batch, fs, ch, chunks=(FS,), gapless=False):
    """decode_loudness over frame slots in calls of the given sizes, flush on
    the last: ([blocks of s], total counts, [peak per call])."""
    dec = handle(batch.n, fs, ch, F=max(chunks))
    got, peaks, a = [[] for _ in range(batch.n)], [], 0
    for i, c in enumerate(chunks):
        offs, sizes = batch.geom(a, a + c)
        blocks = np.full((batch.n, mp3_amd.loud_max_blocks(fs, c)), PATTERN, np.float32)
        blocks, bc, pk, _ = dec.decode_loudness(batch.blob, offs, sizes, c, blocks=blocks, flush=i == len(chunks) - 1,
                                                gapless=gapless)
        for s in range(batch.n):
            assert bc[s] >= 0 and (blocks[s, bc[s]:] == PATTERN).all()
            got[s].append(blocks[s, : bc[s]].copy())
        peaks.append(pk.copy())
        a += c
    rows = [np.concatenate(g) for g in got]
    return rows, np.array([r.shape[0] for r in rows]), peaks


_dec = {}


def decode_case(batch, fs, ch):
    if (fs, ch) not in _dec:
        _dec[(fs, ch)] = decode_chunks(batch, fs, ch)
    return _dec[(fs, ch)]


def packed_on_device(batch, fs, ch, gapless=False):
    """decode_packed(flush) of a fresh handle into device tensors: (dec, out, counts)."""
    dec = handle(batch.n, fs, ch, F=FS)
    offs, sizes = batch.geom(0, FS)
    S = mp3_amd.packed_max_samples(fs, FS)
    out = torch.zeros((batch.n, S, ch), dtype=torch.float32, device="cuda")
    counts = torch.zeros((batch.n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_packed(batch.blob, offs, sizes, FS, out=out, counts=counts, flush=True, gapless=gapless)
    dec.sync()
    return dec, out, counts


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_decode_loudness_is_the_tap_on_the_packed_samples(batch, fs, ch):
    H = block_len(fs)
    rows, bc, peaks = decode_case(batch, fs, ch)
    dec, out, counts = packed_on_device(batch, fs, ch)
    via_tap, tc, tpk = dec.loudness(out, counts, flush=True, stride=mp3_amd.loud_max_blocks(fs, FS))
    dec.sync()
    smp, cnt = out.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(tc, bc) and list(bc) == [int(k) // H for k in cnt]
    assert bc[batch.names.index("empty")] == 0 and bc.max() >= 3
    assert same_bits(tpk, peaks[0])
    worst = 0.0
    for s in range(batch.n):
        assert same_bits(rows[s], via_tap[s, : bc[s]]), batch.names[s]
        x = smp[s, : cnt[s]]
        assert tpk[s] == np.abs(x).max(initial=0.0)
        worst = max(worst, check(rows[s], blocks64(x, fs), x, batch.names[s]))
    print("decoded streams %d Hz x %d: max err/bound %.3g" % (fs, ch, worst))
    # frame by frame: the same blocks within twice the bound
    got, gc, _ = decode_chunks(batch, fs, ch, (1,) * FS)
    assert np.array_equal(gc, bc)
    for s in range(batch.n):
        x = smp[s, : cnt[s]]
        err = np.abs(got[s].astype(np.float64) - rows[s].astype(np.float64))
        assert (err <= 2.0 * bound_of(blocks64(x, fs), x)).all(), batch.names[s]


class Tagged(Batch):
    """The batch plus two streams whose LAME tags trim them."""

    def __init__(self, base):
        import test_gpu_long_packed as LP
        self.names = base.names + ["trim_a", "trim_b"]
        self.streams = base.streams + [LP.trim_stream("a"), LP.trim_stream("b")]
        self.n = len(self.streams)
        self.slots = [mp3_amd.long_plan(d)[0].astype(np.int64) if d else np.zeros(0, np.int64) for d in self.streams]
        self.F = max(len(s) for s in self.slots)
        self.base = np.concatenate([[0], np.cumsum([len(d) for d in self.streams])[:-1]]).astype(np.int64)
        self.blob = np.frombuffer(b"".join(self.streams) + b"\0" * 64, np.uint8)


def test_decode_loudness_gapless(batch):
    fs, ch = 48000, 2
    batch = Tagged(batch)
    _, _, counts = packed_on_device(batch, fs, ch, gapless=True)
    _, _, plain = packed_on_device(batch, fs, ch)
    counts, plain = counts.cpu().numpy(), plain.cpu().numpy()
    assert (counts < plain).any()  # some stream has a LAME tag: its window trims it
    rows, bc, _ = decode_chunks(batch, fs, ch, (5, 11), gapless=True)
    assert list(bc) == [int(k) // block_len(fs) for k in counts]


# ---- lifecycle -------------------------------------------------------------------
def test_stride_overflow():
    fs, ch = 44100, 2
    H = block_len(fs)
    a, b = 3 * H + 7, H + 3
    x = sig(fs, ch, a + b)["noise"]
    dec = handle(3, fs, ch)
    got, bc, pk, raw = tap(dec, [x[:a], x[:b], x[:a]], stride=2)
    assert list(bc) == [-1, 1, -1]
    assert (raw[0] == PATTERN).all() and (raw[2] == PATTERN).all()  # nothing written
    cont = handle(1, fs, ch)
    first, _, _, _ = tap(cont, [x[:b]])
    second, _, _, _ = tap(cont, [x[b:b + a]])
    fresh, _, _, _ = tap(handle(1, fs, ch), [x[b:b + a]])
    nxt, nc, _, _ = tap(dec, [x[b:b + a]] * 3)
    assert same_bits(got[1], first[0]) and same_bits(nxt[1], second[0])  # the stream within the stride goes on
    assert same_bits(nxt[0], fresh[0]) and same_bits(nxt[2], fresh[0])  # the others were restarted
    assert list(nc) == [a // H, (a + b) // H - b // H, a // H]
    got, bc, _, _ = tap(handle(1, fs, ch), [x[:a]], stride=3)  # exactly the need fits
    assert list(bc) == [3]


def test_restarts():
    fs, ch = 48000, 2
    H = block_len(fs)
    x = sig(fs, ch)["noise"]
    a, b = H + 100, 3 * H
    cont = handle(1, fs, ch)
    tap(cont, [x[:a]])
    goes_on, _, _, _ = tap(cont, [x[a:b]])
    fresh, _, _, _ = tap(handle(1, fs, ch), [x[a:b]])
    assert not same_bits(goes_on[0], fresh[0][: goes_on[0].shape[0]])

    def second_call(restart):
        dec = handle(3, fs, ch)
        tap(dec, [x[:a]] * 3)
        restart(dec)
        return tap(dec, [x[a:b]] * 3)[0]

    blob = mp3_amd.BatchDecoder(1, 1).get_state(0, 1)
    for what, restart, slots in [("reset", lambda d: d.reset(), (0, 1, 2)),
                                 ("set_state", lambda d: d.set_state(blob, first=1), (1,)),
                                 ("set_window", lambda d: d.set_window([0], first=1), (1,)),
                                 ("set_loudness", lambda d: d.set_loudness(True), (0, 1, 2))]:
        got = second_call(restart)
        for s in range(3):
            assert same_bits(got[s], fresh[0] if s in slots else goes_on[0]), (what, s)
    dec = handle(1, fs, ch)
    tap(dec, [x[:a]])
    dec.set_output(fs, ch)  # any set_output turns the loudness sink off
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.loudness(x[None, :a], [a])
    dec.set_loudness(True)
    again, _, _, _ = tap(dec, [x[a:b]])
    assert same_bits(again[0], fresh[0])
    dec.set_loudness(False)  # off: the buffers are freed, packed calls still fail or work as before
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.loudness(x[None, :a], [a])


def test_argument_errors(batch):
    fs, ch = 48000, 2
    L = mp3_amd.lib()
    x = sig(fs, ch)["noise"][:5000]
    dec = mp3_amd.BatchDecoder(2, 1)
    assert L.mp3d_batch_set_loudness(dec._h, 1) == -1  # no packed format yet
    dec.set_output(fs, ch)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.loudness(x[None], [5000])  # before set_loudness
    offs, sizes = batch.geom(0, 1)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_loudness(batch.blob, offs[:2], sizes[:2], 1)
    dec.set_loudness(True)
    smp = np.ascontiguousarray(x[None])
    cnt, bc = np.array([5000], np.int32), np.zeros(1, np.int32)
    blocks, pk = np.zeros((1, 4), np.float32), np.zeros(1, np.float32)

    def call(flags, n=1, sp=smp.ctypes.data, bp=blocks.ctypes.data):
        return L.mp3d_batch_loudness(dec._h, sp, 5000, cnt.ctypes.data, n, bp, 4, bc.ctypes.data, pk.ctypes.data, flags,
                                     None)

    assert call(4) == -1  # an unknown flag
    assert call(mp3_amd.PACK_GAPLESS) == -1  # the tap has no frames to read a tag from
    assert call(0, n=3) == -5  # more streams than the handle has
    assert call(0, n=0) == -1
    dsmp = torch.zeros(2 * 5000 * ch + 4, dtype=torch.float32, device="cuda")
    dblk = torch.zeros(16, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert call(0, sp=dsmp.data_ptr() + 2) == -1  # a misaligned device pointer
    assert call(0, bp=dblk.data_ptr() + 1) == -1
    assert call(0) == 0 and bc[0] == 1 and pk[0] == np.abs(x).max()
    assert call(mp3_amd.PACK_FLUSH, sp=dsmp.data_ptr() + 4, bp=dblk.data_ptr() + 4) == 0 and bc[0] == 1
    # device pointers must be int-aligned: counts and block_count as well
    dcnt = torch.tensor([0, 5000, 0, 0], dtype=torch.int32, device="cuda")
    dbc = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call_counts(cp=cnt.ctypes.data, bcp=bc.ctypes.data):
        return L.mp3d_batch_loudness(dec._h, smp.ctypes.data, 5000, cp, 1, blocks.ctypes.data, 4, bcp, pk.ctypes.data,
                                     mp3_amd.PACK_FLUSH, None)

    assert call_counts(cp=dcnt.data_ptr() + 1) == -1 and call_counts(cp=dcnt.data_ptr() + 2) == -1
    assert call_counts(bcp=dbc.data_ptr() + 2) == -1
    bc[0] = -7
    assert call_counts() == 0 and bc[0] == 1
    assert call_counts(cp=dcnt.data_ptr() + 4, bcp=dbc.data_ptr() + 4) == 0
    dec.sync()
    assert dbc.cpu().tolist() == [0, 1, 0, 0]
    lufs = np.zeros(1, np.float32)

    def integrated(cp):
        lufs[0] = 5.0
        return L.mp3d_batch_loudness_integrated(dec._h, blocks.ctypes.data, 4, cp, 1, lufs.ctypes.data, None)

    assert integrated(dcnt.data_ptr() + 1) == -1 and integrated(dcnt.data_ptr() + 2) == -1
    dcnt[1] = 1
    torch.cuda.synchronize()
    assert integrated(bc.ctypes.data) == 0
    want = lufs.copy()
    assert want[0] != 5.0 and integrated(dcnt.data_ptr() + 4) == 0 and same_bits(lufs, want)
    assert L.mp3d_batch_decode_loudness(dec._h, batch.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, 2, 1,
                                        blocks.ctypes.data, 4, bc.ctypes.data, None, 4, None, None) == -1
    with pytest.raises(mp3_amd.MP3DError, match="-5"):
        dec.decode_loudness(batch.blob, offs[:2], sizes[:2], 2)  # more frames than the handle has


@pytest.mark.parametrize("fs,ch", [(48000, 2), (8000, 1)])
def test_host_and_device_buffers_agree(fs, ch):
    lens = tap_lengths(fs)
    name = "quiet after loud"
    want, wc, wpk = tap_case(fs, ch)[name]
    x = sig(fs, ch)[name]
    smp = torch.zeros((6, nmax(fs), ch), dtype=torch.float32, device="cuda")
    for s, k in enumerate(lens):
        smp[s, :k] = torch.from_numpy(x[:k]).cuda()
    strm = torch.cuda.Stream()
    stride = want[-1].shape[0] + 2
    with torch.cuda.stream(strm):
        cnt = torch.tensor(lens, dtype=torch.int32, device="cuda")
        blocks = torch.full((6, stride), float(PATTERN), dtype=torch.float32, device="cuda")
        bc = torch.full((6,), -7, dtype=torch.int32, device="cuda")
        pk = torch.full((6,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dec = handle(6, fs, ch)
        dec.loudness(smp, cnt, blocks=blocks, block_counts=bc, peak=pk, stream=strm.cuda_stream)
    strm.synchronize()
    blocks, bc, pk = blocks.cpu().numpy(), bc.cpu().numpy(), pk.cpu().numpy()
    assert np.array_equal(bc, wc) and same_bits(pk, wpk)
    for s in range(6):
        assert same_bits(blocks[s, : bc[s]], want[s]) and (blocks[s, bc[s]:] == PATTERN).all(), s


def test_integrated_on_the_device():
    fs, ch = 48000, 2
    H = block_len(fs)
    n = 40 * H + 11
    sg = sig(fs, ch, n)
    xs = [sg["sine"], sg["noise"], sg["quiet after loud"], sg["dc step"], sg["noise"][: 3 * H + 5], sg["impulse"]]
    dec = handle(len(xs), fs, ch)
    rows, bc, _, raw = tap(dec, xs)
    assert list(bc) == [40, 40, 40, 40, 3, 40]
    bc = bc.copy()
    bc[5] = -1  # an overflowed row
    got = dec.integrated_lufs(raw, bc)
    assert got.dtype == np.float32 and got[4] == -np.inf and got[5] == -np.inf
    for s in range(4):
        want = mp3_amd.integrated_lufs(rows[s])
        assert abs(want - integrated64(rows[s].astype(np.float64))) <= 1e-9
        assert np.isfinite(want) and abs(float(got[s]) - want) <= 1e-4, (s, got[s], want)
    # two loud blocks: G[0] and G[1] hold 2/4 and 1/4 of them, the quiet rest is gated out (ungated: -17 LU)
    assert got[1] - 5.5 < got[2] < got[1] - 3.0
    d_raw, d_bc = torch.from_numpy(raw).cuda(), torch.from_numpy(bc).cuda()
    d_out = torch.zeros(len(xs), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dec.integrated_lufs(d_raw, d_bc, lufs=d_out)
    dec.sync()
    assert same_bits(d_out.cpu().numpy(), got)


def test_loudness_time(batch):
    dec = handle(batch.n, 48000, 2, F=FS)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.loudness_time_us()  # no loudness call yet
    offs, sizes = batch.geom(0, FS)
    dec.decode_loudness(batch.blob, offs, sizes, FS, flush=True)
    assert dec.loudness_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- poison ----------------------------------------------------------------------
def assert_same_case(batch, fs, ch):
    for name, (got, bc, pk) in run_tap_case(fs, ch).items():
        want, wc, wpk = tap_case(fs, ch)[name]
        assert np.array_equal(bc, wc) and same_bits(pk, wpk), name
        assert all(same_bits(a, b) for a, b in zip(got, want)), name
    rows, bc, peaks = decode_chunks(batch, fs, ch)
    want, wc, wpeaks = decode_case(batch, fs, ch)
    assert np.array_equal(bc, wc) and same_bits(peaks[0], wpeaks[0])
    for s in range(batch.n):
        assert same_bits(rows[s], want[s]), batch.names[s]


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_poison(batch, fs, ch, monkeypatch):
    tap_case(fs, ch), decode_case(batch, fs, ch)  # (the product library's, without the poison)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    assert_same_case(batch, fs, ch)


@pytest.mark.parametrize("fs,ch", [(48000, 2), (11025, 1)])
def test_workgroup_lds_poison_build(batch, fs, ch, monkeypatch):
    tap_case(fs, ch), decode_case(batch, fs, ch)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        assert_same_case(batch, fs, ch)
