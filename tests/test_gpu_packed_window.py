"""GPU: per-stream sample windows of the packed and the feature sink
(MP3D_PACK_GAPLESS, BatchDecoder.set_window / sink_window; include/mp3d.h
"Sample windows").

The oracle of the gapless flag is the long-stream sink: a windowed stream of
the batched sink must equal decode_long_packed(gapless=True) of the same bytes
bit for bit, because both stage the same kept samples for the same rs_tile
(DESIGN.md section 4b).  Explicit windows are compared with the float64
reference of tests/test_gpu_packed.py on x[lo:hi], within that file's bound.

The nine-stream batch: trim_stream("a") .. ("f") of tests/
test_gpu_long_packed.py, the untagged c3_s0, an empty stream and the untagged
lsf_22k_js.  (b) keeps 47 samples of its first audio frame (fewer than T - 1)
and is cut 971 samples inside its last; (c), LSF, skips three whole frames and
501 samples and loses 319 samples plus its last two frames; (d) has its end
past the data, (e) no frame count, (f) its start past the data.
"""
import numpy as np
import pytest

import _golden
import mp3_amd
import test_gpu_features as FT
import test_gpu_long_packed as LP
import test_gpu_packed as PK
from mp3_amd import _build
from test_long_packed import audio_stream

pytestmark = pytest.mark.gpu

NO_END = mp3_amd.WINDOW_NO_END
FORMATS = [(48000, 2), (16000, 1), (44100, 2)]
TAGGED = list("abcdef")


class Batch(PK.Batch):
    """PK.Batch's layout (geom) over a list of streams of one's own."""

    def __init__(self, names, streams):
        self.names, self.streams, self.n = names, streams, len(streams)
        self.slots = [mp3_amd.long_plan(d)[0].astype(np.int64) if d else np.zeros(0, np.int64) for d in streams]
        self.F = max(len(s) for s in self.slots)
        self.base = np.concatenate([[0], np.cumsum([len(d) for d in streams])[:-1]]).astype(np.int64)
        self.blob = np.frombuffer(b"".join(streams) + b"\0" * 64, np.uint8)


@pytest.fixture(scope="module")
def nine():
    names = TAGGED + ["c3_s0", "empty", "lsf_22k_js"]
    streams = [LP.trim_stream(w) for w in TAGGED] + [LP.golden("c3_s0"), b"", audio_stream("lsf_22k_js")]
    b = Batch(names, streams)
    assert b.n == 9 and b.F <= 42
    return b


def plain_of(batch, s):
    """(rows, infos, StreamInfo) of stream s from decode_long, or None for the
    empty one; computed once per stream."""
    name = batch.names[s]
    if not batch.streams[s]:
        return None
    return LP.plain(("trim_" if name in TAGGED else "window_") + name, batch.streams[s])


def tag_window(si):
    if not si.has_lame:
        return 0, NO_END
    return si.skip_samples, si.end_sample if si.end_sample >= 0 else NO_END


def run(batch, fmt, f32=True, chunks=None, gapless=True, windows=None, tail_flush=False, stride=None):
    """Decode frame slots [0, sum(chunks)) in calls of the given sizes; the
    last call flushes, or with tail_flush one more call whose sizes are all 0.
    gapless: one value or one per call.  Returns (samples per stream, handle)."""
    chunks = chunks or [batch.F]
    flags = gapless if isinstance(gapless, list) else [gapless] * len(chunks)
    dec = mp3_amd.BatchDecoder(batch.n, max(chunks))
    dec.set_output(*fmt)
    if windows is not None:
        dec.set_window([w[0] for w in windows], [w[1] for w in windows])
    got = [[] for _ in range(batch.n)]
    calls = [(a, c, g) for a, c, g in zip(np.cumsum([0] + chunks[:-1]), chunks, flags)]
    if tail_flush:
        calls.append((sum(chunks), 1, flags[-1]))
    for i, (a, c, g) in enumerate(calls):
        offs, sizes = batch.geom(int(a), int(a) + c)
        if tail_flush and i == len(calls) - 1:
            assert not sizes.any()
        out, counts, _ = dec.decode_packed(batch.blob, offs, sizes, c, f32=f32, flush=i == len(calls) - 1, gapless=g,
                                           stride=stride)
        for s in range(batch.n):
            assert counts[s] >= 0, (batch.names[s], i)
            got[s].append(out[s, : counts[s]].copy())
    return [np.concatenate(g) for g in got], dec


_whole, _long = {}, {}


def whole(batch, fmt, f32, gapless=True):
    """The nine streams in one flushed call; computed once per case."""
    key = (fmt, f32, gapless)
    if key not in _whole:
        _whole[key] = run(batch, fmt, f32=f32, gapless=gapless)[0]
    return _whole[key]


def long_ref(which, fmt, f32):
    key = (which, fmt, f32)
    if key not in _long:
        _long[key] = LP.long_run(LP.trim_stream(which), fmt, f32=f32, gapless=True)[0]
    return _long[key]


def chunkings(F):
    return [5, 11, F - 16], [1] * F


# ---- the fixtures are what the cases above say they are -------------------------
def test_the_windows_the_tags_give(nine):
    _, dec = run(nine, (48000, 2))
    lo, hi, fed = dec.sink_window()
    want = {"a": (1105, None), "b": (1105, 45109), "c": (2229, 7745), "d": (1105, 60 * 1152 + 529 - 1500),
            "e": (1105, NO_END), "f": (2529, 1 * 1152 + 529), "c3_s0": (0, NO_END), "empty": (0, NO_END),
            "lsf_22k_js": (0, NO_END)}
    for s, name in enumerate(nine.names):
        p = plain_of(nine, s)
        n = int(p[1]["samples"].sum()) if p else 0
        assert fed[s] == n, name
        assert lo[s] == want[name][0], name
        if want[name][1] is not None:
            assert hi[s] == want[name][1], name
        if p:
            assert (lo[s], hi[s]) == tag_window(p[2]), name
    n = dict(zip(nine.names, fed))
    assert n["b"] == 40 * 1152 and n["b"] - hi[1] == 971 and 1152 - lo[1] == 47
    assert n["c"] == 16 * 576 and lo[2] == 3 * 576 + 501 and n["c"] - hi[2] == 319 + 2 * 576
    assert hi[3] > n["d"] and lo[5] > n["f"] == 1152
    T = mp3_amd.resample_filter(44100, 16000)[2].shape[1]
    assert 47 < T - 1


# ---- 1. bits against the long-stream sink ---------------------------------------
@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("fmt", FORMATS)
def test_gapless_equals_the_long_sink(nine, fmt, f32):
    got = whole(nine, fmt, f32)
    bare = whole(nine, fmt, f32, gapless=False)
    for s, name in enumerate(nine.names):
        if name not in TAGGED:
            LP.same_bits(got[s], bare[s], name)  # untagged: the flag changes nothing
            continue
        LP.same_bits(got[s], long_ref(name, fmt, f32), (name, fmt, f32))
        rows, infos, si = plain_of(nine, s)
        n_trim = mp3_amd.gapless_trim(mp3_amd.pcm_to_planar(rows, infos), si).shape[1]
        hz = int(infos["hz"][infos["samples"] > 0][0])
        L, M = PK.filt(hz, fmt[0])[:2]
        print("%s %s f32=%d: N' %d, %d samples" % (name, fmt, f32, n_trim, len(got[s])))
        assert len(got[s]) == -(-n_trim * L // M), name
        assert len(got[s]) < len(bare[s])
    assert len(got[nine.names.index("f")]) == 0 and len(got[nine.names.index("empty")]) == 0


# ---- 2. split calls --------------------------------------------------------------
@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("fmt", FORMATS)
def test_split_calls_are_bit_identical(nine, fmt, f32):
    want = whole(nine, fmt, f32)
    split, single = chunkings(nine.F)
    for chunks, tail in ((split, False), (single, False), (single, True)):
        got = run(nine, fmt, f32=f32, chunks=chunks, tail_flush=tail)[0]
        for s, name in enumerate(nine.names):
            LP.same_bits(got[s], want[s], (name, fmt, f32, len(chunks), tail))


# ---- 3. FFmpeg -------------------------------------------------------------------
def test_gapless_int16_matches_ffmpeg(nine):
    ref = np.load(_golden.GOLDEN / "keypress_128k_js.tagged.pcm16.npy")
    got = whole(nine, (44100, 2), False)[0]
    assert got.T.shape == ref.shape, (got.T.shape, ref.shape)
    assert int(np.abs(got.T.astype(np.int32) - ref.astype(np.int32)).max()) <= 1


# ---- 4. the flag is latched at the first fed sample ------------------------------
@pytest.mark.parametrize("fmt", [(48000, 2), (16000, 1)])
def test_flag_is_latched_by_the_first_fed_sample(nine, fmt):
    F = nine.F
    for s in range(6):  # slot 0 of every tagged stream is its tag frame: the first call feeds nothing
        assert plain_of(nine, s)[1]["samples"][0] == 0
    # the flag only on the call that holds the tag frame: nothing is trimmed
    got = run(nine, fmt, chunks=[1, 1, F - 2], gapless=[True, False, True])[0]
    for g, w, name in zip(got, whole(nine, fmt, True, gapless=False), nine.names):
        LP.same_bits(g, w, name)
    # the flag from the second call on: trimmed
    got = run(nine, fmt, chunks=[1, 1, F - 2], gapless=[False, True, False])[0]
    for g, w, name in zip(got, whole(nine, fmt, True), nine.names):
        LP.same_bits(g, w, name)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_flush_is_not_a_stream_start(nine, fmt):
    K = 5
    dec = mp3_amd.BatchDecoder(nine.n, nine.F)
    dec.set_output(*fmt)
    offs, sizes = nine.geom(0, K)
    dec.decode_packed(nine.blob, offs, sizes, K, flush=True, gapless=True)
    lo, hi, fed = dec.sink_window()
    offs, sizes = nine.geom(K, nine.F)
    out, counts, _ = dec.decode_packed(nine.blob, offs, sizes, nine.F - K, flush=True, gapless=True)
    lo2, hi2, fed2 = dec.sink_window()
    exact = 0
    for s, name in enumerate(nine.names):
        p = plain_of(nine, s)
        if p is None:
            assert (lo[s], hi[s], fed[s], counts[s]) == (0, NO_END, 0, 0)
            continue
        rows, infos, si = p
        r1 = int(infos["samples"][:K].sum())
        assert r1 > 0 and fed[s] == r1 and (lo[s], hi[s]) == tag_window(si), name
        assert (lo2[s], hi2[s]) == (lo[s], hi[s]) and fed2[s] == int(infos["samples"].sum()), name
        hz, x = PK.mapped_input(rows, infos, fmt[1])
        rest = x[max(int(lo[s]), r1):max(min(int(hi[s]), len(x)), r1)]  # of the TRIMMED signal, started fresh
        y, bound = PK.reference(rest, hz, fmt[0])
        got = out[s, : counts[s]]
        assert counts[s] == y.shape[0], (name, counts[s], y.shape)
        err = float(np.abs(got.astype(np.float64) - y).max()) if y.size else 0.0
        print("%s %s: %d samples after the flush, max err %.3g, bound %.3g" % (name, fmt, counts[s], err, bound))
        assert err <= bound, name
        if hz == fmt[0] and set(infos["channels"][infos["samples"] > 0]) == {fmt[1]}:
            LP.same_bits(got, np.ascontiguousarray(rest), name)
            exact += 1
    assert fmt != (44100, 2) or exact >= 5


# ---- 5. explicit windows ---------------------------------------------------------
WINDOWS = [(1152, 2304), (0, 1), (1151, 1153), (0, 0), (500, 500), (10 ** 6, None), (777, None), (0, None),
           (100, 10 ** 7), (1151, 1153), (1152, 2304), (0, 1), (777, None)]


@pytest.fixture(scope="module")
def thirteen():
    b = PK.Batch()
    assert b.n == len(WINDOWS)
    return b


@pytest.fixture(scope="module")
def thirteen_plain(thirteen):
    return PK.make_plain(thirteen)


_explicit = {}


def explicit(batch, fmt):
    if fmt not in _explicit:
        _explicit[fmt] = run(batch, fmt, gapless=False, windows=WINDOWS)[0]
    return _explicit[fmt]


@pytest.mark.parametrize("fmt", FORMATS)
def test_explicit_windows(thirteen, thirteen_plain, fmt):
    rows, infos = thirteen_plain
    got = explicit(thirteen, fmt)
    exact = 0
    for s, name in enumerate(thirteen.names):
        hz, x = PK.mapped_input(rows[s], infos[s], fmt[1])
        lo, hi = WINDOWS[s]
        xw = x[lo:hi]
        if s in (5, 8):
            assert lo > len(x) or hi > len(x)  # past the stream
        y, bound = PK.reference(xw, hz, fmt[0]) if hz else (np.zeros((0, fmt[1])), 0.0)
        assert len(got[s]) == y.shape[0], (name, len(got[s]), y.shape)
        err = float(np.abs(got[s].astype(np.float64) - y).max()) if y.size else 0.0
        print("%s %s [%s, %s): %d samples, max err %.3g, bound %.3g" % (fmt, name, lo, hi, len(got[s]), err, bound))
        assert err <= bound, name
        chans = {int(c) for c, k in zip(infos[s]["channels"], infos[s]["samples"]) if k}
        if hz == fmt[0] and chans == {fmt[1]}:
            LP.same_bits(got[s], np.ascontiguousarray(xw), name)
            exact += len(xw) > 0
    assert fmt != (44100, 2) or exact >= 2
    # split calls
    F = thirteen.F
    chunks = [5, 11, F - 16] if F > 16 else [5, F - 5]
    for g, w, name in zip(run(thirteen, fmt, chunks=chunks, gapless=False, windows=WINDOWS)[0], got, thirteen.names):
        LP.same_bits(g, w, name)
    # an explicit window beats the flag (keypress_128k_js carries a LAME tag)
    flagged, dec = run(thirteen, fmt, gapless=True, windows=WINDOWS)
    for g, w, name in zip(flagged, got, thirteen.names):
        LP.same_bits(g, w, name)
    k = thirteen.names.index("keypress_128k_js")
    assert dec.stream_info(thirteen.n)[k].has_lame == 1 and WINDOWS[k] == (777, None)
    lo, hi, _ = dec.sink_window()
    assert [(int(a), None if b == NO_END else int(b)) for a, b in zip(lo, hi)] == WINDOWS


# ---- 6. a crop from the middle of a file -----------------------------------------
def test_crop_from_the_middle_of_a_file():
    data = LP.golden("long_c3_512")
    off, seg, _ = mp3_amd.long_plan(data, 1)
    j = 300
    j0 = int(seg[j])
    assert 0 < j0 < j  # a real warm-up
    lo = (j - j0) * 1152 + 100
    F = j - j0 + 2
    chunk = data[int(off[j0]):int(off[j0 + F])]
    dec = mp3_amd.BatchDecoder(1, F)
    dec.set_output(44100, 2)
    dec.set_window([lo], [lo + 2000])
    out, counts, infos = dec.decode_packed(np.frombuffer(chunk + b"\0" * 64, np.uint8), [0], [len(chunk)], F, flush=True)
    assert (infos[0]["samples"][: j - j0] == 1152).all() and (infos[0]["hz"] == 44100).all()
    rows, _, _ = LP.plain("long_c3_512", data)
    want = np.ascontiguousarray(rows[j:j + 2].reshape(-1, 2)[100:2100])
    assert counts[0] == 2000
    LP.same_bits(out[0, :2000], want)


# ---- 7. features -----------------------------------------------------------------
def test_gapless_features(nine):
    def handle(F):
        dec = mp3_amd.BatchDecoder(nine.n, F)
        dec.set_output(16000, 1)
        dec.set_features(80)
        return dec

    xs = [long_ref(name, (16000, 1), True)[:, 0] if name in TAGGED else whole(nine, (16000, 1), True)[s][:, 0]
          for s, name in enumerate(nine.names)]
    want, want_counts, _ = FT.tap(handle(1), xs, flush=True)
    offs, sizes = nine.geom()
    feat, counts, _ = handle(nine.F).decode_features(nine.blob, offs, sizes, nine.F, flush=True, gapless=True)
    for s, name in enumerate(nine.names):
        assert counts[s] == want_counts[s] == FT.ceil_frames(len(xs[s])), name
        assert FT.same_bits(feat[s, : counts[s]], want[s]), name
    assert counts[0] > 0 and counts[nine.names.index("f")] == 0
    # single-frame calls
    dec = handle(1)
    got = [[] for _ in range(nine.n)]
    for a in range(nine.F):
        offs, sizes = nine.geom(a, a + 1)
        f1, c1, _ = dec.decode_features(nine.blob, offs, sizes, 1, flush=a == nine.F - 1, gapless=True)
        for s in range(nine.n):
            assert c1[s] >= 0
            got[s].append(f1[s, : c1[s]].copy())
    for s, name in enumerate(nine.names):
        assert FT.same_bits(np.concatenate(got[s]), want[s]), name


# ---- 8. restart rules and errors -------------------------------------------------
def test_restart_rules(nine):
    B = nine.names.index("b")
    fixed = (1105, 45109, 4 * 1152)
    unfixed = (0, NO_END, 0)

    def at(dec, s=B):
        lo, hi, fed = dec.sink_window(s, 1)
        return int(lo[0]), int(hi[0]), int(fed[0])

    def start():
        dec = mp3_amd.BatchDecoder(nine.n, 8)
        dec.set_output(48000, 2)
        assert at(dec) == unfixed
        offs, sizes = nine.geom(0, 5)
        dec.decode_packed(nine.blob, offs, sizes, 5, gapless=True)
        assert at(dec) == fixed
        return dec

    dec = start()
    offs, sizes = nine.geom(nine.F, nine.F + 1)
    dec.decode_packed(nine.blob, offs, sizes, 1, flush=True)  # a flush is no window restart
    assert at(dec) == fixed
    dec.reset()
    assert at(dec) == unfixed
    dec = start()
    dec.set_state(mp3_amd.BatchDecoder(1, 1).get_state(0, 1), first=B)
    assert at(dec) == unfixed and at(dec, 0)[::2] == (1105, 4 * 1152)  # the other slots are left alone
    dec = start()
    dec.set_output(48000, 2)
    assert at(dec) == unfixed
    dec = start()
    dec.set_window(None)
    assert at(dec) == unfixed and at(dec, 0) == unfixed
    dec = start()
    dec.set_window([7], [9], first=B)  # a window restart of one slot
    assert at(dec) == (7, 9, 0) and at(dec, 0)[::2] == (1105, 4 * 1152)
    # a stride overflow restarts the resampler, not the window, and still counts
    dec = start()
    offs, sizes = nine.geom(5, 13)
    _, counts, _ = dec.decode_packed(nine.blob, offs, sizes, 8, stride=1000)
    assert counts[B] == -1
    assert at(dec) == (1105, 45109, 12 * 1152)


def test_errors(nine):
    L = mp3_amd.lib()
    lo, hi = np.array([3], np.int64), np.array([9], np.int64)
    dec = mp3_amd.BatchDecoder(nine.n, 8)
    assert L.mp3d_batch_set_window(dec._h, 0, 1, lo.ctypes.data, hi.ctypes.data) == -1  # before set_output
    dec.set_output(48000, 2)
    dec.set_window([3], [9], first=2)
    before = [a.copy() for a in dec.sink_window()]
    bad = [(np.array([-1], np.int64), hi), (np.array([10], np.int64), hi)]
    for s in (0, 2):
        for blo, bhi in bad:
            assert L.mp3d_batch_set_window(dec._h, s, 1, blo.ctypes.data, bhi.ctypes.data) == -1
        assert L.mp3d_batch_set_window(dec._h, s, 1, None, hi.ctypes.data) == -1
    two = np.array([0, -1], np.int64)  # one bad element: nothing is written
    assert L.mp3d_batch_set_window(dec._h, 0, 2, two.ctypes.data, None) == -1
    for a, b in zip(before, dec.sink_window()):
        assert np.array_equal(a, b)
    assert before[0][2] == 3 and before[1][2] == 9
    assert L.mp3d_batch_set_window(dec._h, nine.n, 1, lo.ctypes.data, hi.ctypes.data) == -5
    assert L.mp3d_batch_set_window(dec._h, nine.n - 1, 2, None, None) == -5
    assert L.mp3d_batch_sink_window(dec._h, nine.n, 1, lo.ctypes.data, None, None) == -5
    with pytest.raises(ValueError):
        dec.set_window([3], [2])
    # flag bit 4 is still refused
    offs, sizes = nine.geom(0, 5)
    out = np.zeros((nine.n, 8192, 2), np.float32)
    cnt = np.zeros(nine.n, np.int32)
    for flags, rc in ((4, -1), (4 | 2, -1), (8, -1), (2, 0)):
        assert L.mp3d_batch_decode_packed(dec._h, nine.blob.ctypes.data, offs.ctypes.data, sizes.ctypes.data, nine.n, 5,
                                          out.ctypes.data, 1, 8192, cnt.ctypes.data, flags, None, None) == rc, flags


# ---- 9. poison -------------------------------------------------------------------
def poison_cases(nine, thirteen):
    out = []
    for fmt in FORMATS:
        for f32 in (True, False):
            out += run(nine, fmt, f32=f32)[0]
        out += run(thirteen, fmt, gapless=False, windows=WINDOWS)[0]
    return out


def test_poison(nine, thirteen, monkeypatch):
    want = poison_cases(nine, thirteen)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    got = poison_cases(nine, thirteen)
    assert len(got) == len(want)
    for w, g in zip(want, got):
        LP.same_bits(g, w)


def test_workgroup_lds_poison_build(nine, thirteen):
    want = poison_cases(nine, thirteen)
    with mp3_amd.library(_build.WGLDS_LIB):
        got = poison_cases(nine, thirteen)
    for w, g in zip(want, got):
        LP.same_bits(g, w)
