"""GPU: the segment sink (BatchDecoder.set_segments / set_segment_threshold /
segments / decode_segments / long_segments; include/mp3d.h "segment sink").

Reference: the header's definition in numpy (tests/test_segment_host.py
segments_ref and segments_by_call).  After one float32 quantisation every
operation of the definition is integer arithmetic, so every comparison here is
on exact lists and counts; there is no tolerance.  One batch per format and
parameter set holds every mask class, every stream length and every value
class; its reference is computed once.

The signals made from hop masks sit on the threshold: an active hop has every
sample at +-q0 / 32768 with thr = H q0^2, so E == thr exactly, and an inactive
hop differs from it in one sample at q0 - 1, so E == thr - (2 q0 - 1).
"""
import re

import numpy as np
import pytest
import torch

import _golden
import mp3_amd
from mp3_amd import _build
from test_gpu_features import FS, Batch
from test_gpu_loudness import Tagged
from test_segment_host import hop, keypress, segments_by_call, segments_ref

pytestmark = pytest.mark.gpu

FORMATS = [(48000, 2), (44100, 2), (22050, 1), (11025, 1), (8000, 1)]
PARAMS = [(1, 1, 0), (5, 3, 2), (30, 10, 5), (256, 256, 128)]
PATTERN = np.int64(-777)
Q0 = 1000
TILE = int(re.search(r"^#define MP3D_SG_TILE\s+(\d+)", (_build.CSRC / "mp3d_segment.h").read_text(), re.M).group(1))


# ---- signals ----------------------------------------------------------------------
def on(k):
    return [True] * k


def off(k):
    return [False] * k


def mask_classes(P, S, rng):
    """{name: hop mask}; every mask but at_zero_and_end ends in silence long enough to emit without a flush"""
    rest = off(P + S + 2)
    s1 = max(S // 2, 1)
    s2 = max(S - s1 - (P - 1), 1)
    rnd = []
    while len(rnd) < min(3 * (S + P), 600):
        rnd += on(int(rng.integers(1, 2 * S + 2))) + off(int(rng.integers(1, 2 * P + 2)))
    return {
        "gap_filled": off(2) + on(S) + off(P - 1) + on(S) + rest,  # a pause of P - 1: one segment
        "gap_split": off(2) + on(S) + off(P) + on(S) + rest,  # of P: two
        "burst_dropped": off(1) + on(S - 1) + rest,
        "burst_kept": off(1) + on(S) + rest,
        "joined": off(1) + on(s1) + off(P - 1) + on(s2) + rest,  # two short bursts, kept: fill comes before drop
        "lead_trail": off(P - 1) + on(S) + off(P - 1),  # silence of P - 1 at either end is not filled
        "at_zero_and_end": on(S + 1) + off(P) + on(S),  # pad clipped at 0, end clipped to N at a flush
        "all_on": on(S + P + 3),
        "all_off": off(S + P + 3),
        "random": rnd,
    }


def mask_signal(mask, fs, ch, n=None):
    """float32 [n, ch] (n defaults to the mask's whole hops) with a[b] == mask[b] at thr = H Q0^2, every hop within
    2 Q0 - 1 of the threshold; in stereo the channels differ by 0.5 and only their mix carries the signal"""
    H = hop(fs)
    q = np.full((len(mask), H), Q0, np.int64)
    q[:, 1::2] = -Q0
    q[~np.asarray(mask, bool), H // 2] = Q0 - 1
    v = (q.reshape(-1)[: len(mask) * H if n is None else n] / 32768.0).astype(np.float32)
    if ch == 1:
        return v[:, None]
    return np.stack([v + np.float32(0.25), v - np.float32(0.25)], axis=1)  # (exact, and so is their sum)


def noise_signal(fs, ch, n, rng):
    """uniform noise, runs of hops at amplitude 0.1 (-25 dBFS) and at 1e-4 (-85 dBFS), for the default -40 dBFS"""
    H = hop(fs)
    amp = []
    while len(amp) * H < n + H:
        amp += [0.1] * int(rng.integers(1, 40)) + [1e-4] * int(rng.integers(1, 60))
    x = rng.uniform(-1.0, 1.0, (len(amp) * H, ch)) * np.repeat(amp, H)[:, None]
    return x[:n].astype(np.float32)


def lens(fs, P, S):
    H = hop(fs)
    return [0, 1, H - 1, H, H + 1, (S + P) * H - 1, (S + P) * H + 1, TILE * H - 1, TILE * H, TILE * H + 1,
            3 * TILE * H + 17]


def streams(fs, ch, P, S):
    """[(name, x float32 [n, ch], thr)] of the format's batch"""
    H = hop(fs)
    rng = np.random.default_rng(97 + fs + ch + 1000 * P + S)
    out = [(k, mask_signal(m, fs, ch), H * Q0 * Q0) for k, m in mask_classes(P, S, rng).items()]
    cut = mask_classes(P, S, rng)["random"]
    out.append(("random_cut", mask_signal(cut, fs, ch, len(cut) * H - H // 3), H * Q0 * Q0))
    dflt = mp3_amd.segment_threshold(fs, -40.0)
    out += [("noise_%d" % n, noise_signal(fs, ch, n, rng), dflt) for n in lens(fs, P, S)]
    # full scale and beyond: -1 and -2 clamp to -32768 and E == H 2^30 == thr; +1 and +2 clamp to 32767, under it
    m = np.array(off(1) + on(S) + off(P) + on(S + 1) + off(S + P + 1), bool)
    for peak in (1.0, 2.0):
        v = np.repeat(np.where(m, -peak, peak), H).astype(np.float32)
        out.append(("full_%g" % peak, np.repeat(v[:, None], ch, 1), H * 2 ** 30))
    if ch == 2:  # both channels loud, the mix silent
        v = rng.uniform(0.5, 0.9, (S + P + 3) * H).astype(np.float32)
        out.append(("left_is_minus_right", np.stack([v, -v], axis=1), dflt))
    return out


_streams, _ref, _case = {}, {}, {}


def batch_of(fs, ch, P, S):
    key = (fs, ch, P, S)
    if key not in _streams:
        _streams[key] = streams(fs, ch, P, S)
        for _, x, _ in _streams[key]:
            x.setflags(write=False)
    return _streams[key]


def ref(fs, ch, P, S, pad, flush):
    """[segments of stream s] of the batch fed to fresh slots in one call: computed once, never changed"""
    key = (fs, ch, P, S, pad, flush)
    if key not in _ref:
        _ref[key] = [segments_ref(x, fs, thr, P, S, pad, flush) for _, x, thr in batch_of(fs, ch, P, S)]
    return _ref[key]


# ---- the stage --------------------------------------------------------------------
def handle(n, fs, ch, P, S, pad, thr=None, F=1):
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_output(fs, ch)
    dec.set_segments(True, min_pause_ms=10 * P, min_speech_ms=10 * S, pad_ms=10 * pad)
    if thr is not None:
        dec.set_segment_threshold(energy=thr)
    return dec


def feed(dec, xs, flush=False, stride=None):
    """Feed xs[s] ([k, ch]) to stream s in one call; returns ([segments of s], counts, raw seg)."""
    n, (fs, ch) = len(xs), dec._out
    P, S = dec._segments
    ss = max(1, max(len(x) for x in xs))
    smp = np.zeros((n, ss, ch), np.float32)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = x
    cnt = np.array([len(x) for x in xs], np.int32)
    stride = stride if stride is not None else mp3_amd.segment_max(fs, ss, P, S)
    seg = np.full((n, stride, 2), PATTERN, np.int64)
    seg, sc = dec.segments(smp, cnt, seg=seg, flush=flush)
    for s in range(n):
        assert (seg[s, max(int(sc[s]), 0):] == PATTERN).all(), s  # nothing past the count is touched
    return [[tuple(p) for p in seg[s, : max(int(sc[s]), 0)].tolist()] for s in range(n)], sc, seg


def run_case(fs, ch, P, S, pad):
    """{flush: (segments, counts)} of the batch in one call on fresh slots"""
    b = batch_of(fs, ch, P, S)
    xs, thr = [x for _, x, _ in b], [t for _, _, t in b]
    return {flush: feed(handle(len(b), fs, ch, P, S, pad, thr), xs, flush=flush)[:2] for flush in (True, False)}


def case(fs, ch, P, S, pad):
    key = (fs, ch, P, S, pad)
    if key not in _case:
        _case[key] = run_case(fs, ch, P, S, pad)
    return _case[key]


@pytest.mark.parametrize("fs,ch", FORMATS)
@pytest.mark.parametrize("P,S,pad", PARAMS)
def test_values(fs, ch, P, S, pad):
    """Every mask class, stream length and value class in one call, flushed and not: the lists and the counts."""
    H = hop(fs)
    names = [k for k, _, _ in batch_of(fs, ch, P, S)]
    for flush in (True, False):
        got, sc = case(fs, ch, P, S, pad)[flush]
        want = ref(fs, ch, P, S, pad, flush)
        for s, name in enumerate(names):
            what = "%d Hz x %d, P %d S %d pad %d, %s, flush %d" % (fs, ch, P, S, pad, name, flush)
            assert sc[s] == len(want[s]) and got[s] == want[s], what
    # what the classes are there to show, on the flushed lists
    w = dict(zip(names, ref(fs, ch, P, S, pad, True)))
    assert len(w["gap_filled"]) == 1 and len(w["gap_split"]) == 2 and len(w["burst_kept"]) == 1
    assert w["burst_dropped"] == [] and w["all_off"] == [] and len(w["joined"]) == 1
    assert w["lead_trail"] == [(max(P - 1 - pad, 0) * H, min(P - 1 + S + pad, 2 * P - 2 + S) * H)]
    assert w["at_zero_and_end"] == [(0, (S + 1 + pad) * H), ((S + 1 + P - pad) * H, (2 * S + 1 + P) * H)]
    assert w["all_on"] == [(0, (S + P + 3) * H)] and ref(fs, ch, P, S, pad, False)[names.index("all_on")] == []
    assert len(w["full_1"]) == 2 and w["full_1"] == w["full_2"]
    if ch == 2:
        assert w["left_is_minus_right"] == []
    assert any(w["noise_%d" % n] for n in lens(fs, P, S))


@pytest.mark.parametrize("fs,ch", FORMATS)
def test_split_invariance(fs, ch):
    """Two streams in calls of 1, H - 1, 997 samples and whole tiles with empty calls in between, cut at different
    places: each call emits exactly the segments the emit rule assigns to it."""
    P, S, pad = 5, 3, 2
    H = hop(fs)
    rng = np.random.default_rng(fs)
    masks = [mask_classes(P, S, rng)["random"] * 16 for _ in (0, 1)]
    n = min(len(m) for m in masks) * H - 7
    xs = [mask_signal(m, fs, ch, n) for m in masks]
    sizes = [[1, 0, H - 1, 0, 997, TILE * H, 0], [997, TILE * H, 0, 1, 0, 0, H - 1]]
    cuts, pos = [[], []], [0, 0]
    while min(pos) < n:
        for s in (0, 1):
            pos[s] = min(pos[s] + sizes[s][len(cuts[s]) % 7], n)
            cuts[s].append(pos[s])
    cuts = [c + [n] for c in cuts]  # the last call feeds nothing and flushes
    want = [segments_by_call(xs[s], fs, H * Q0 * Q0, P, S, pad, cuts[s], True) for s in (0, 1)]
    dec = handle(2, fs, ch, P, S, pad, [H * Q0 * Q0] * 2)
    at, total = [0, 0], [[], []]
    for i in range(len(cuts[0])):
        got, sc, _ = feed(dec, [xs[s][at[s]: cuts[s][i]] for s in (0, 1)], flush=i == len(cuts[0]) - 1)
        for s in (0, 1):
            assert got[s] == want[s][i], (s, i)
            total[s] += got[s]
            at[s] = cuts[s][i]
    for s in (0, 1):
        assert total[s] == segments_ref(xs[s], fs, H * Q0 * Q0, P, S, pad, True) and len(total[s]) > 10
        assert sum(len(w) > 0 for w in want[s][:-1]) > 3  # segments come out along the way, not only at the flush


@pytest.mark.parametrize("fs,ch,shift", [(48000, 2, 2), (48000, 2, 1), (44100, 2, 3), (11025, 1, 1), (8000, 1, 3)])
def test_strided_input(fs, ch, shift):
    """Samples that start `shift` floats into their allocation (one stereo frame, half a stereo frame, an odd
    number of mono frames): rows that no 16-byte load meets at its first sample."""
    P, S, pad = 5, 3, 2
    H = hop(fs)
    xs = [mask_signal(sum((on(S + (k + r) % 3) + off(P + k % 2) for k in range(10 + r)), off(r)), fs, ch)
          for r in (0, 1, 2)]
    ss = max(len(x) for x in xs) + 1  # (an odd stride: the rows start at different offsets of 16 bytes)
    flat = torch.zeros(shift + 3 * ss * ch, dtype=torch.float32, device="cuda")
    smp = flat[shift:].view(3, ss, ch)
    for s, x in enumerate(xs):
        smp[s, : len(x)] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    assert smp.data_ptr() == flat.data_ptr() + 4 * shift
    seg, sc = handle(3, fs, ch, P, S, pad, [H * Q0 * Q0] * 3).segments(smp, [len(x) for x in xs], flush=True)
    for s, x in enumerate(xs):
        want = segments_ref(x, fs, H * Q0 * Q0, P, S, pad, True)
        assert sc[s] == len(want) > 3 and [tuple(p) for p in seg[s, : sc[s]].tolist()] == want, s


def test_one_long_stream():
    """40 tiles at n_streams = 1: the energy tiles are independent, one stream spreads over the GPU."""
    fs, ch, P, S, pad = 48000, 2, 30, 10, 5
    H = hop(fs)
    n = 40 * TILE * H - 3
    x = noise_signal(fs, ch, n, np.random.default_rng(40))
    got, sc, _ = feed(handle(1, fs, ch, P, S, pad), [x], flush=True)
    want = segments_ref(x, fs, mp3_amd.segment_threshold(fs, -40.0), P, S, pad, True)
    assert -(-n // (TILE * H)) == 40 and got[0] == want and len(want) > 5


# ---- overflow and restarts --------------------------------------------------------
def test_stride_overflow():
    fs, ch, P, S, pad = 44100, 2, 5, 3, 2
    H = hop(fs)
    thr = [H * Q0 * Q0] * 3
    burst = on(S) + off(P)
    a = mask_signal(burst * 4 + off(S + P), fs, ch)  # four segments emitted without a flush
    b = mask_signal(off(1) + burst * 2 + off(S + P), fs, ch)
    short = mask_signal(burst + on(2), fs, ch)  # ends inside a run: nothing emitted yet
    need = len(segments_ref(a, fs, thr[0], P, S, pad, False))
    assert need == 4 and segments_ref(short, fs, thr[0], P, S, pad, False) == []
    dec = handle(3, fs, ch, P, S, pad, thr)
    got, sc, raw = feed(dec, [a, short, a], stride=need - 1)
    assert list(sc) == [-1, 0, -1] and (raw == PATTERN).all()  # nothing written
    fresh, _, _ = feed(handle(1, fs, ch, P, S, pad, thr[:1]), [b])
    cont = handle(1, fs, ch, P, S, pad, thr[:1])
    feed(cont, [short])
    second, _, _ = feed(cont, [b])
    nxt, _, _ = feed(dec, [b] * 3)
    assert nxt[0] == fresh[0] and nxt[2] == fresh[0]  # the two were restarted
    assert nxt[1] == second[0] and second[0] != fresh[0] and len(fresh[0]) == 2  # the third goes on
    got, sc, _ = feed(handle(1, fs, ch, P, S, pad, thr[:1]), [a], stride=need)  # exactly the need fits
    assert list(sc) == [need]
    got, sc, raw = feed(handle(1, fs, ch, P, S, pad, thr[:1]), [a], stride=0)
    assert list(sc) == [-1]


def test_restarts():
    """Every restart of the definition: the slot then answers as a fresh one does, the others go on, and the
    threshold survives."""
    fs, ch, P, S, pad = 11025, 1, 5, 3, 2
    H = hop(fs)
    thr = H * Q0 * Q0
    a = mask_signal(off(2) + on(S + 4), fs, ch, (S + 6) * H - 5)  # ends inside a run, inside a hop
    b = mask_signal(on(3) + off(P) + on(S) + off(P + S + 1), fs, ch)
    fresh, _, _ = feed(handle(1, fs, ch, P, S, pad, [thr]), [b])
    cont = handle(1, fs, ch, P, S, pad, [thr])
    feed(cont, [a])
    goes_on, _, _ = feed(cont, [b])
    assert len(fresh[0]) == 2 and len(goes_on[0]) == 2 and goes_on[0] != fresh[0]
    # (at the default threshold the signal's hops are all active: the custom one is what splits them)
    assert feed(handle(1, fs, ch, P, S, pad), [b])[0][0] == []

    def primed(n=2):
        dec = handle(n, fs, ch, P, S, pad, [thr] * n)
        feed(dec, [a] * n)
        return dec

    def expect(dec, restarted):
        got, _, _ = feed(dec, [b] * len(restarted))
        for s, r in enumerate(restarted):
            assert got[s] == (fresh[0] if r else goes_on[0]), (s, r)

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
    dec.set_segment_threshold(energy=[thr], first=1)
    expect(dec, [False, True])
    dec = primed()
    tail, sc, _ = feed(dec, [a[:0], a[:7]], flush=True)  # its own flush restarts both
    assert list(sc) == [1, 1] and tail[0] == [(0, len(a))] and tail[1] == [(0, len(a) + 7)]
    expect(dec, [True, True])
    dec = primed()
    dec.set_segments(True, min_pause_ms=10 * P, min_speech_ms=10 * S, pad_ms=10 * pad)  # the thresholds are the default's again
    assert feed(dec, [b] * 2)[0] == [[], []]
    dec = primed()
    dec.set_output(fs, ch)  # turns the sink off
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.segments(np.ascontiguousarray(a[None]), [len(a)])
    dec.set_segments(True, min_pause_ms=10 * P, min_speech_ms=10 * S, pad_ms=10 * pad)
    dec.set_segment_threshold(energy=[thr] * 2)
    expect(dec, [True, True])
    # the other sinks' states are not this one's: a limiter call in between changes nothing
    dec = primed()
    dec.set_limiter(True, -1.0)
    dec.limit(np.ascontiguousarray(a[None]), [len(a)])
    expect(dec, [False, False])


def test_argument_errors(batch):
    fs, ch = 48000, 2
    L = mp3_amd.lib()
    H = hop(fs)
    x = np.ascontiguousarray(noise_signal(fs, ch, 5000, np.random.default_rng(3))[None])
    dec = mp3_amd.BatchDecoder(2, 1)
    assert L.mp3d_batch_set_segments(dec._h, 1, 30, 10, 5) == -1  # no packed format yet
    dec.set_output(fs, ch)
    cnt, sc = np.array([5000, 0], np.int32), np.zeros(2, np.int32)
    seg = np.zeros((2, 8, 2), np.int64)
    one = np.array([1], np.uint64)

    def call(flags=0, n=1, sp=x.ctypes.data, gp=seg.ctypes.data, cp=cnt.ctypes.data, scp=sc.ctypes.data, stride=5000,
             gstride=8):
        return L.mp3d_batch_segments(dec._h, sp, stride, cp, n, gp, gstride, scp, flags, None)

    assert call() == -1  # before set_segments
    assert L.mp3d_batch_set_segment_threshold(dec._h, 0, 1, one.ctypes.data) == -1
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.segments(x, [5000])
    offs, sizes = batch.geom(0, 1)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_segments(batch.blob, offs[:2], sizes[:2], 1)
    for P, S, pad in [(0, 10, 0), (257, 10, 0), (30, 0, 0), (30, 257, 0), (30, 10, -1), (30, 10, 16), (1, 1, 1)]:
        assert L.mp3d_batch_set_segments(dec._h, 1, P, S, pad) == -1, (P, S, pad)
    assert call() == -1  # refused parameters leave the sink off
    assert L.mp3d_batch_set_segments(dec._h, 1, 256, 256, 128) == 0 and L.mp3d_batch_set_segments(dec._h, 1, 1, 1, 0) == 0
    dec.set_segments(True)
    assert dec._segments == (30, 10)
    for bad in (0, H * 2 ** 30 + 1):
        assert L.mp3d_batch_set_segment_threshold(dec._h, 0, 1, np.array([bad], np.uint64).ctypes.data) == -1, bad
    full = np.array([H * 2 ** 30, 1], np.uint64)
    assert L.mp3d_batch_set_segment_threshold(dec._h, 0, 2, full.ctypes.data) == 0
    assert L.mp3d_batch_set_segment_threshold(dec._h, 1, 2, full.ctypes.data) == -5
    assert L.mp3d_batch_set_segment_threshold(dec._h, -1, 1, one.ctypes.data) == -1
    assert L.mp3d_batch_set_segment_threshold(dec._h, 0, 0, one.ctypes.data) == -1
    assert L.mp3d_batch_set_segment_threshold(dec._h, 0, 1, None) == -1
    with pytest.raises(ValueError):
        dec.set_segment_threshold()
    dec.set_segment_threshold(db=-30.0, n=2)
    assert call(4) == -1 and call(mp3_amd.PACK_GAPLESS) == -1  # unknown flag; the stage has no frames to read a tag from
    assert call(n=3) == -5 and call(n=0) == -1
    assert call(sp=None) == -1 and call(gp=None) == -1 and call(cp=None) == -1 and call(scp=None) == -1
    assert call(stride=-1) == -1 and call(gstride=-1) == -1 and call(stride=2 ** 31 - 1) == -1 and call(gstride=2 ** 31) == -1
    dsmp = torch.zeros(2 * 5000 * ch + 4, dtype=torch.float32, device="cuda")
    dseg = torch.zeros(2 * 8 * 2 + 2, dtype=torch.int64, device="cuda")
    dcnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert call(sp=dsmp.data_ptr() + 2) == -1  # misaligned device pointers
    assert call(gp=dseg.data_ptr() + 4) == -1  # a device seg is aligned to 8 bytes
    assert call(scp=dcnt.data_ptr() + 2) == -1 and call(cp=dcnt.data_ptr() + 1) == -1
    assert call(sp=dsmp.data_ptr() + 4, gp=dseg.data_ptr() + 8, scp=dcnt.data_ptr() + 4) == 0
    assert call(mp3_amd.PACK_FLUSH) == 0
    dec.sync()

    def decode(flags=0, n=2, F=1, gp=seg.ctypes.data, scp=sc.ctypes.data):
        return L.mp3d_batch_decode_segments(dec._h, batch.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, n, F,
                                            gp, 8, scp, flags, None, None)

    assert decode(4) == -1 and decode(gp=None) == -1 and decode(scp=None) == -1 and decode(n=3) == -5
    assert decode(F=2) == -5 and decode(n=0) == -1
    assert decode(mp3_amd.PACK_FLUSH | mp3_amd.PACK_GAPLESS) == 0
    with pytest.raises(mp3_amd.MP3DError, match="set_segments"):
        mp3_amd.BatchDecoder(1, 1).long_segments(b"")


@pytest.mark.parametrize("fs,ch,P,S,pad", [(48000, 2, 5, 3, 2), (8000, 1, 30, 10, 5)])
def test_host_and_device_buffers_agree(fs, ch, P, S, pad):
    b = batch_of(fs, ch, P, S)
    n, ss = len(b), max(1, max(len(x) for _, x, _ in b))
    thr = [t for _, _, t in b]
    smp = torch.zeros((n, ss, ch), dtype=torch.float32, device="cuda")
    for s, (_, x, _) in enumerate(b):
        smp[s, : len(x)] = torch.from_numpy(x.copy()).cuda()
    stride = mp3_amd.segment_max(fs, ss, P, S)
    strm = torch.cuda.Stream()
    for flush in (True, False):
        want, wc = case(fs, ch, P, S, pad)[flush]
        with torch.cuda.stream(strm):
            cnt = torch.tensor([len(x) for _, x, _ in b], dtype=torch.int32, device="cuda")
            seg = torch.full((n, stride, 2), int(PATTERN), dtype=torch.int64, device="cuda")
            got = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dec = handle(n, fs, ch, P, S, pad, thr)
            dec.segments(smp, cnt, seg=seg, seg_counts=got, flush=flush, stream=strm.cuda_stream)
        strm.synchronize()
        seg, got = seg.cpu().numpy(), got.cpu().numpy()
        for s in range(n):
            assert got[s] == wc[s] and [tuple(p) for p in seg[s, : got[s]].tolist()] == want[s], (s, flush)
            assert (seg[s, got[s]:] == PATTERN).all()
        mixed, mc = handle(n, fs, ch, P, S, pad, thr).segments(smp, cnt, flush=flush)  # device in, host out
        for s in range(n):
            assert mc[s] == got[s] and np.array_equal(mixed[s, : mc[s]], seg[s, : got[s]])


# ---- composition ------------------------------------------------------------------
DEC_FMT = (48000, 2)
DEC_PARAMS = (5, 3, 2)


@pytest.fixture(scope="module")
def batch():
    return Tagged(Batch())


def median_thresholds(batch, smp, counts):
    """each stream's median hop energy (at least 1): masks that flip often"""
    from test_segment_host import hop_energy, quantise
    H = hop(DEC_FMT[0])
    thr = []
    for s in range(batch.n):
        E = hop_energy(quantise(smp[s, : counts[s]]), H, True)
        thr.append(max(int(np.median(E)) if len(E) else 1, 1))
    return thr


@pytest.mark.parametrize("gapless", [False, True])
def test_decode_segments_is_the_stage_on_the_packed_samples(batch, gapless):
    fs, ch = DEC_FMT
    P, S, pad = DEC_PARAMS
    offs, sizes = batch.geom(0, FS)
    pk = mp3_amd.BatchDecoder(batch.n, FS)
    pk.set_output(fs, ch)
    dout = torch.zeros((batch.n, mp3_amd.packed_max_samples(fs, FS), ch), dtype=torch.float32, device="cuda")
    dcnt = torch.zeros(batch.n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pk.decode_packed(batch.blob, offs, sizes, FS, out=dout, counts=dcnt, flush=True, gapless=gapless)
    pk.sync()
    smp, counts = dout.cpu().numpy(), dcnt.cpu().numpy()
    thr = median_thresholds(batch, smp, counts)
    via, vc = handle(batch.n, fs, ch, P, S, pad, thr).segments(dout, dcnt, flush=True)  # on the device output
    assert vc[batch.names.index("empty")] == 0 and (vc > 1).any()
    for chunks in ((FS,), (5, 11)):
        dec = handle(batch.n, fs, ch, P, S, pad, thr, F=max(chunks))
        got, a = [[] for _ in range(batch.n)], 0
        for i, c in enumerate(chunks):
            o, z = batch.geom(a, a + c)
            seg, sc, _ = dec.decode_segments(batch.blob, o, z, c, flush=i == len(chunks) - 1, gapless=gapless)
            for s in range(batch.n):
                assert sc[s] >= 0
                got[s] += [tuple(p) for p in seg[s, : sc[s]].tolist()]
            a += c
        for s in range(batch.n):
            assert got[s] == [tuple(p) for p in via[s, : vc[s]].tolist()], (batch.names[s], chunks)
    for s in range(batch.n):  # and the definition itself, on decoded audio
        assert [tuple(p) for p in via[s, : vc[s]].tolist()] == segments_ref(smp[s, : counts[s]], fs, thr[s], P, S, pad, True)


def test_the_keypress_fixture(batch):
    """The decoded file at 44.1 kHz stereo, gapless, -40 dBFS, (5, 3, 2): one segment (0, 9702), the list
    tests/test_segment_host.py computes from the fixture, whose hops all clear the threshold by more than one LSB
    per sample could move them; long_segments gives the same list for the same file."""
    fs, ch = 44100, 2
    s = batch.names.index("keypress_128k_js")
    offs, sizes = batch.geom()
    dec = handle(batch.n, fs, ch, 5, 3, 2, F=batch.F)
    seg, sc, _ = dec.decode_segments(batch.blob, offs, sizes, batch.F, flush=True, gapless=True)
    assert sc[s] == 1 and tuple(seg[s, 0]) == (0, 9702)
    assert segments_ref(keypress(), fs, mp3_amd.segment_threshold(fs, -40.0), 5, 3, 2, True) == [(0, 9702)]
    one = handle(8, fs, ch, 5, 3, 2, F=32 + 11)  # (a long decode's segments of 32 frames and their warm-up)
    lseg, pcm, si, in_hz = one.long_segments(_golden.case("keypress_128k_js")[0])
    assert lseg.dtype == np.int64 and lseg.tolist() == [[0, 9702]] and in_hz == 44100
    assert pcm.is_cuda and tuple(pcm.shape) == (len(keypress()), ch)
    # and on another file, against the batch path at a threshold that splits it
    name = "c5_dual_32k_vbr"
    t = batch.names.index(name)
    smp, counts, _ = dec.decode_packed(batch.blob, offs, sizes, batch.F, flush=True, gapless=True)
    thr = median_thresholds(batch, smp, counts)[t]
    both = handle(batch.n, fs, ch, 5, 3, 2, [thr] * batch.n, F=batch.F)
    seg, sc, _ = both.decode_segments(batch.blob, offs, sizes, batch.F, flush=True, gapless=True)
    one.set_segment_threshold(energy=[thr])
    lseg, pcm, _, _ = one.long_segments(batch.streams[t])
    assert len(pcm) == counts[t] and lseg.tolist() == seg[t, : sc[t]].tolist() and sc[t] > 0


def test_segment_time(batch):
    fs, ch = DEC_FMT
    dec = handle(batch.n, fs, ch, *DEC_PARAMS, F=FS)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.segment_time_us()  # no segment call yet
    offs, sizes = batch.geom(0, FS)
    dec.decode_segments(batch.blob, offs, sizes, FS, flush=True)
    assert dec.segment_time_us() > 0.0 and dec.resample_time_us() > 0.0


# ---- poison -----------------------------------------------------------------------
def assert_same_case(fs, ch, P, S, pad):
    got, want = run_case(fs, ch, P, S, pad), case(fs, ch, P, S, pad)
    for key in want:
        assert got[key][0] == want[key][0] and np.array_equal(got[key][1], want[key][1]), key


def test_poison(monkeypatch):
    args = (48000, 2, 30, 10, 5)
    case(*args)  # (the product library's, without the poison)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    assert_same_case(*args)


def test_workgroup_lds_poison_build(monkeypatch):
    args = (11025, 1, 5, 3, 2)
    case(*args)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    with mp3_amd.library(_build.WGLDS_LIB):
        assert_same_case(*args)
