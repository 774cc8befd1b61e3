"""GPU: the packed uniform-rate PCM sink (BatchDecoder.set_output /
decode_packed; include/mp3d.h "packed uniform-rate PCM sink").

One ragged batch: 16-frame goldens of both MPEG families (stereo, dual, mono,
CRC, 8 / 16 / 22.05 / 32 / 44.1 / 48 kHz), the tagged keypress stream, an
empty stream and a 5 x 7 mixed-corpus batch.  The expected output is built
from the decoder's own plain float32 rows of a fresh handle (pinned to FFmpeg
and the oracle by the rest of the suite): concatenated per infos, channel
mapped in float32, filtered in float64 with the taps of resample_filter.

Value bound: the sink accumulates T products in one float32 FMA chain, so a
sample is within gamma_T * sum_j |taps[p][j] x[j]| <= (T + 2) * 2^-24 * S * A
of the float64 sum, S = max_p sum_j |taps[p][j]|, A = the stream's peak input.
"""
import numpy as np
import pytest
import torch

import _gen
import _golden
import mp3_amd

pytestmark = pytest.mark.gpu

GOLD = ["c3_s0", "c5_mono_48k_crc", "c5_dual_32k_vbr", "lsf_22k_js", "lsf_8k_js", "lsf_16k_mono_crc",
        "keypress_128k_js"]
FORMATS = [(48000, 2), (16000, 1), (44100, 2)]


class Batch:
    def __init__(self):
        streams = [_golden.case(nm)[0] for nm in GOLD] + [b""]
        buf, offs, sizes = _gen.batch(_gen.C5, 4242, 5, 7)
        streams += [bytes(buf[offs[s]:offs[s] + sizes[s]]) for s in range(5)]
        self.names = GOLD + ["empty"] + ["c5_%d" % s for s in range(5)]
        self.streams = streams
        self.n = len(streams)
        # frame slots of every stream (host walk): byte offset of each slot
        self.slots = [mp3_amd.long_plan(d)[0].astype(np.int64) if d else np.zeros(0, np.int64) for d in streams]
        self.F = max(len(s) for s in self.slots)
        self.base = np.concatenate([[0], np.cumsum([len(d) for d in streams])[:-1]]).astype(np.int64)
        self.blob = np.frombuffer(b"".join(streams) + b"\0" * 64, np.uint8)

    def geom(self, a=0, b=None):
        """offsets / sizes of frame slots [a, b) of every stream."""
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


def mapped_input(rows, infos, out_ch):
    """(in_hz, x float32 [N, out_ch]) of one stream from its plain rows."""
    parts, hz = [], 0
    for f in range(rows.shape[0]):
        k, ch = int(infos[f]["samples"]), int(infos[f]["channels"])
        if not k:
            continue
        hz = hz or int(infos[f]["hz"])
        x = rows[f, : k * ch].reshape(k, ch)
        if ch == 2 and out_ch == 1:
            x = (np.float32(0.5) * (x[:, 0] + x[:, 1]))[:, None]
        elif ch == 1 and out_ch == 2:
            x = np.repeat(x, 2, axis=1)
        parts.append(x.astype(np.float32))
    if not parts:
        return 0, np.zeros((0, out_ch), np.float32)
    return hz, np.concatenate(parts)


def filt(hz, out_hz):
    if hz == out_hz:
        return 1, 1, np.ones((1, 1), np.float32), 0, 0
    L, M, taps = mp3_amd.resample_filter(hz, out_hz)
    T = taps.shape[1]
    return L, M, taps, T // 2 - 1, T // 2


def emitted(n, L, M, post):
    return -(-(n - post) * L // M) if n > post else 0


def reference(x, hz, out_hz):
    """float64 y [ceil(N L / M), ch] and the error bound per sample."""
    L, M, taps, pre, post = filt(hz, out_hz)
    T = taps.shape[1]
    N = x.shape[0]
    cnt = -(-N * L // M)
    xp = np.concatenate([np.zeros((pre, x.shape[1])), x.astype(np.float64), np.zeros((post + 1, x.shape[1]))])
    y = np.zeros((cnt, x.shape[1]))
    t64 = taps.astype(np.float64)
    for a in range(0, cnt, 8192):
        m = np.arange(a, min(cnt, a + 8192), dtype=np.int64)
        n0, p = (m * M) // L, (m * M) % L
        idx = n0[:, None] + np.arange(T)[None, :]  # x[n0 - pre + j] in the padded array
        y[a:a + m.size] = np.einsum("mt,mtc->mc", t64[p], xp[idx])
    S = float(np.abs(t64).sum(axis=1).max())
    A = float(np.abs(x).max()) if N else 0.0
    return y, (T + 2) * 2.0 ** -24 * S * A


def make_plain(batch):
    """Plain float32 rows and infos of the whole batch from a fresh handle."""
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    offs, sizes = batch.geom()
    return dec.decode(batch.blob, offs, sizes, batch.F, f32=True)


def make_expected(batch, plain, formats=FORMATS):
    """{(out_hz, out_ch): [(y float64, bound)] per stream}."""
    rows, infos = plain
    out = {}
    for hz_o, ch_o in formats:
        per = []
        for s in range(batch.n):
            hz, x = mapped_input(rows[s], infos[s], ch_o)
            per.append(reference(x, hz, hz_o) if hz else (np.zeros((0, ch_o)), 0.0))
        out[(hz_o, ch_o)] = per
    return out


@pytest.fixture(scope="module")
def plain(batch):
    return make_plain(batch)


@pytest.fixture(scope="module")
def expected(batch, plain):
    """Computed once."""
    return make_expected(batch, plain)


PATTERN = np.float32(-777.25)


def run_whole(batch, fmt, f32=True, stride=None, dec=None):
    dec = dec or mp3_amd.BatchDecoder(batch.n, batch.F)
    dec.set_output(*fmt)
    stride = stride or mp3_amd.packed_max_samples(fmt[0], batch.F)
    out = np.full((batch.n, stride, fmt[1]), PATTERN if f32 else -1234, np.float32 if f32 else np.int16)
    offs, sizes = batch.geom()
    out, counts, infos = dec.decode_packed(batch.blob, offs, sizes, batch.F, out=out, f32=f32, flush=True)
    return out, counts, infos


def check_values(batch, expected, fmt, out, counts):
    for s in range(batch.n):
        y, bound = expected[fmt][s]
        assert counts[s] == y.shape[0], (batch.names[s], counts[s], y.shape)
        got = out[s, : counts[s]].astype(np.float64)
        err = float(np.abs(got - y).max()) if y.size else 0.0
        print("%s %s: %d samples, max err %.3g, bound %.3g" % (fmt, batch.names[s], counts[s], err, bound))
        assert err <= bound, (batch.names[s], err, bound)
        assert (out[s, counts[s]:] == PATTERN).all(), batch.names[s]  # nothing past the samples is touched
    assert counts[batch.names.index("empty")] == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_values_and_counts(batch, expected, fmt):
    out, counts, infos = run_whole(batch, fmt)
    check_values(batch, expected, fmt, out, counts)


@pytest.mark.parametrize("fmt", FORMATS)
def test_poison(batch, expected, fmt, monkeypatch):
    ref_out, ref_counts, _ = run_whole(batch, fmt)
    monkeypatch.setenv("MP3D_DEBUG_POISON", "1")
    out, counts, _ = run_whole(batch, fmt)
    check_values(batch, expected, fmt, out, counts)
    assert np.array_equal(counts, ref_counts) and np.array_equal(out.view(np.uint32), ref_out.view(np.uint32))


def test_bypass_is_a_copy(batch, plain):
    rows, infos = plain
    seen = 0
    for fmt in [(44100, 2), (48000, 1), (32000, 2), (22050, 2), (8000, 2), (16000, 1)]:
        out, counts, _ = run_whole(batch, fmt)
        for s in range(batch.n):
            hz, x = mapped_input(rows[s], infos[s], fmt[1])
            chans = {int(c) for c, k in zip(infos[s]["channels"], infos[s]["samples"]) if k}
            if hz != fmt[0] or chans != {fmt[1]}:
                continue
            seen += 1
            assert counts[s] == x.shape[0]
            assert np.array_equal(out[s, : counts[s]].view(np.uint32), x.view(np.uint32)), (fmt, batch.names[s])
    assert seen >= 7


def run_chunks(batch, fmt, chunks, f32=True):
    """Decode frame slots [0, sum(chunks)) in calls of the given sizes, flush
    on the last call only; returns (concatenated samples per stream, counts
    per call)."""
    dec = mp3_amd.BatchDecoder(batch.n, max(chunks))
    dec.set_output(*fmt)
    got = [[] for _ in range(batch.n)]
    per_call = []
    a = 0
    for i, c in enumerate(chunks):
        offs, sizes = batch.geom(a, a + c)
        out, counts, _ = dec.decode_packed(batch.blob, offs, sizes, c, f32=f32, flush=i == len(chunks) - 1)
        for s in range(batch.n):
            assert counts[s] >= 0
            got[s].append(out[s, : counts[s]].copy())
        per_call.append(counts.copy())
        a += c
    return [np.concatenate(g) for g in got], per_call


@pytest.mark.parametrize("fmt", FORMATS)
def test_chunking_is_bit_identical(batch, plain, fmt):
    rows, infos = plain
    runs = [run_chunks(batch, fmt, ch) for ch in ([16], [5, 11], [1] * 16)]
    for s in range(batch.n):
        for r in runs[1:]:
            assert np.array_equal(r[0][s].view(np.uint32), runs[0][0][s].view(np.uint32)), (fmt, batch.names[s])
    # per-call counts: the emit rule on the inputs seen so far
    for (_, per_call), chunks in zip(runs, ([16], [5, 11], [1] * 16)):
        for s in range(batch.n):
            hz = next((int(i["hz"]) for i in infos[s][:16] if i["samples"]), 0)
            if not hz:
                assert all(c[s] == 0 for c in per_call)
                continue
            L, M, taps, pre, post = filt(hz, fmt[0])
            seen, done, a = 0, 0, 0
            for i, c in enumerate(chunks):
                seen += int(infos[s]["samples"][a:a + c].sum())
                a += c
                total = -(-seen * L // M) if i == len(chunks) - 1 else emitted(seen, L, M, post)
                assert per_call[i][s] == total - done, (fmt, batch.names[s], i)
                done = total


@pytest.mark.parametrize("fmt", FORMATS)
def test_int16_sink(batch, fmt):
    f, cf, _ = run_whole(batch, fmt, f32=True)
    q, cq, _ = run_whole(batch, fmt, f32=False)
    assert np.array_equal(cf, cq)
    for s in range(batch.n):
        assert np.array_equal(q[s, : cq[s]], _golden.to_int16(f[s, : cf[s]])), batch.names[s]
        assert (q[s, cq[s]:] == -1234).all()


def test_state_rules(batch):
    fmt = (48000, 2)
    fresh, fresh_counts, _ = run_whole(batch, fmt)
    F = batch.F
    offs5, sizes5 = batch.geom(0, 5)

    def same_as_fresh(out, counts, streams=range(batch.n)):
        for s in streams:
            assert counts[s] == fresh_counts[s], batch.names[s]
            assert np.array_equal(out[s, : counts[s]].view(np.uint32), fresh[s, : counts[s]].view(np.uint32)), s

    # reset: the resamplers restart with the decoder state
    dec = mp3_amd.BatchDecoder(batch.n, F)
    dec.set_output(*fmt)
    dec.decode_packed(batch.blob, offs5, sizes5, 5)
    dec.reset()
    same_as_fresh(*run_whole(batch, fmt, dec=dec)[:2])
    # set_state onto a slot: a seek is a discontinuity (slot 0 to the stream start)
    dec = mp3_amd.BatchDecoder(batch.n, F)
    dec.set_output(*fmt)
    dec.decode_packed(batch.blob, offs5, sizes5, 5)
    dec.set_state(mp3_amd.BatchDecoder(1, 1).get_state(0, 1), first=0)
    same_as_fresh(*run_whole(batch, fmt, dec=dec)[:2], streams=[0])
    # after a flush, and after a change of the output format, the next output
    # starts like a fresh resampler: compare with a handle that reached the
    # same decoder state (5 frames in) by a plain call
    offs11, sizes11 = batch.geom(5, 16)
    b = mp3_amd.BatchDecoder(batch.n, 11)
    b.set_output(*fmt)
    b.decode(batch.blob, offs5, sizes5, 5, f32=True)
    out_b, cnt_b, _ = b.decode_packed(batch.blob, offs11, sizes11, 11, flush=True)
    assert cnt_b.max() > 0
    for first_fmt, flush in ((fmt, True), ((16000, 1), False)):
        a = mp3_amd.BatchDecoder(batch.n, 11)
        a.set_output(*first_fmt)
        a.decode_packed(batch.blob, offs5, sizes5, 5, flush=flush)
        if first_fmt != fmt:
            a.set_output(*fmt)
        out_a, cnt_a, _ = a.decode_packed(batch.blob, offs11, sizes11, 11, flush=True)
        assert np.array_equal(cnt_a, cnt_b)
        for s in range(batch.n):
            assert np.array_equal(out_a[s, : cnt_a[s]].view(np.uint32), out_b[s, : cnt_b[s]].view(np.uint32)), s
    # a plain call after packed calls continues the streams bit-identically
    p = mp3_amd.BatchDecoder(batch.n, 11)
    p.decode(batch.blob, offs5, sizes5, 5, f32=True)
    want, want_inf = p.decode(batch.blob, offs11, sizes11, 11, f32=True)
    h = mp3_amd.BatchDecoder(batch.n, 11)
    h.set_output(16000, 1)
    h.decode_packed(batch.blob, offs5, sizes5, 5)
    got, got_inf = h.decode(batch.blob, offs11, sizes11, 11, f32=True)
    assert np.array_equal(got_inf, want_inf) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_off_and_on_again(batch, expected):
    """The sink turned off (its buffers freed) and on again with the same
    format: the same flushed call, on a reset decoder state, gives the bits of
    a fresh handle."""
    fmt = (48000, 2)
    fresh, fresh_counts, _ = run_whole(batch, fmt)
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    for turn in range(2):
        out, counts, _ = run_whole(batch, fmt, dec=dec)  # (sets the format: on)
        assert np.array_equal(counts, fresh_counts), turn
        assert np.array_equal(out.view(np.uint32), fresh.view(np.uint32)), turn
        dec.set_output(0, 0)
        dec.reset()  # the decoder state only: the sink is off
    check_values(batch, expected, fmt, out, counts)


def test_stride_overflow(batch, expected):
    """Stride = the bound for 16 frames of MPEG-1 input: a stream whose output
    exceeds it gets -1, writes nothing and restarts; the others are
    unaffected.  (Of the 16-frame LSF streams only the 8 kHz one exceeds it at
    48 kHz: 16 kHz mono gives 27 648 and 22.05 kHz 20 063 of the 27 684.)"""
    fmt = (48000, 2)
    stride = mp3_amd.packed_max_samples(48000, 16, 32000)
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    out, counts, infos = run_whole(batch, fmt, stride=stride, dec=dec)
    over = [s for s in range(batch.n) if expected[fmt][s][0].shape[0] > stride]
    assert batch.names.index("lsf_8k_js") in over
    for s in over:
        assert batch.names[s].startswith("lsf_")  # every MPEG-1 stream is unaffected
        assert counts[s] == -1 and (out[s] == PATTERN).all()
    for s in range(batch.n):
        if s in over:
            continue
        y, bound = expected[fmt][s]
        assert counts[s] == y.shape[0]
        assert np.abs(out[s, : counts[s]] - y).max(initial=0.0) <= bound
        assert (out[s, counts[s]:] == PATTERN).all()
    # the next flushed call with a full stride starts like a fresh resampler
    dec.reset()
    out2, counts2, _ = run_whole(batch, fmt, dec=dec)
    fresh, fresh_counts, _ = run_whole(batch, fmt)
    assert np.array_equal(counts2, fresh_counts)
    for s in over:
        assert np.array_equal(out2[s, : counts2[s]].view(np.uint32), fresh[s, : counts2[s]].view(np.uint32))
    # ... and without a reset of the decoder: the overflowed stream's resampler
    # restarted, its decoder state advanced (compare with a plain call first)
    s8 = batch.names.index("lsf_8k_js")
    offs, sizes = batch.geom(0, 8)
    offs2, sizes2 = batch.geom(8, 16)
    a = mp3_amd.BatchDecoder(batch.n, 8)
    a.set_output(*fmt)
    _, ca, _ = a.decode_packed(batch.blob, offs, sizes, 8, stride=1000)
    assert ca[s8] == -1
    oa, ca, _ = a.decode_packed(batch.blob, offs2, sizes2, 8, flush=True)
    b = mp3_amd.BatchDecoder(batch.n, 8)
    b.set_output(*fmt)
    b.decode(batch.blob, offs, sizes, 8, f32=True)
    ob, cb, _ = b.decode_packed(batch.blob, offs2, sizes2, 8, flush=True)
    assert ca[s8] == cb[s8] > 0
    assert np.array_equal(oa[s8, : ca[s8]].view(np.uint32), ob[s8, : cb[s8]].view(np.uint32))


@pytest.mark.parametrize("fmt", [(48000, 2), (16000, 1)])
@pytest.mark.parametrize("f32", [True, False])
def test_device_pointers_on_a_callers_stream(batch, f32, fmt):
    """Every argument a torch tensor: the kernel's own stores land in the
    caller's buffer, so the pattern past each stream's samples also checks
    them (upsampling stereo and the general, downsampling mono path)."""
    want, want_counts, want_infos = run_whole(batch, fmt, f32=f32)
    stride = want.shape[1]
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    dec.set_output(*fmt)
    offs, sizes = batch.geom()
    strm = torch.cuda.Stream()
    with torch.cuda.stream(strm):
        d_in = torch.from_numpy(batch.blob.copy()).cuda()
        out = torch.full((batch.n, stride, fmt[1]), float(PATTERN) if f32 else -1234,
                         dtype=torch.float32 if f32 else torch.int16, device="cuda")
        counts = torch.full((batch.n,), -7, dtype=torch.int32, device="cuda")
        infos = torch.zeros((batch.n, batch.F, 6), dtype=torch.int32, device="cuda")
        dec.decode_packed(d_in, offs, sizes, batch.F, out=out, counts=counts, infos=infos, f32=f32, flush=True,
                          stream=strm.cuda_stream)
    strm.synchronize()
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert np.array_equal(out.cpu().numpy(), want)  # the untouched pattern included
    got_infos = infos.cpu().numpy().reshape(-1).view(mp3_amd.FRAME_INFO_DT).reshape(batch.n, batch.F)
    assert np.array_equal(got_infos, want_infos)


def test_misaligned_device_sink_is_refused(batch):
    """A device sink must be aligned to one sample frame (mp3d.h)."""
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    dec.set_output(48000, 2)
    offs, sizes = batch.geom()
    stride = mp3_amd.packed_max_samples(48000, batch.F)
    flat = torch.zeros(batch.n * stride * 2 + 1, dtype=torch.float32, device="cuda")
    out = flat[1:].view(batch.n, stride, 2)  # 4 bytes off an 8-byte frame
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_packed(batch.blob, offs, sizes, batch.F, out=out, flush=True)
    assert not flat.any().item()


def test_error_paths(batch):
    offs, sizes = batch.geom()
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_packed(batch.blob, offs, sizes, batch.F)
    L = mp3_amd.lib()
    for hz, ch in [(44000, 2), (96000, 1), (48000, 3), (48000, 0), (-1, 1)]:
        assert L.mp3d_batch_set_output(dec._h, hz, ch) == -1
    dec.set_output(48000, 2)
    dec.decode_packed(batch.blob, offs, sizes, batch.F, flush=True)
    dec.set_output(0, 0)  # off: the buffers are freed, packed calls refused, plain calls work
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        dec.decode_packed(batch.blob, offs, sizes, batch.F)
    dec.reset()
    pcm, infos = dec.decode(batch.blob, offs, sizes, batch.F, f32=True)
    want, want_infos = mp3_amd.BatchDecoder(batch.n, batch.F).decode(batch.blob, offs, sizes, batch.F, f32=True)
    assert np.array_equal(infos, want_infos) and np.array_equal(pcm.view(np.uint32), want.view(np.uint32))


def test_resample_time(batch):
    dec = mp3_amd.BatchDecoder(batch.n, batch.F)
    dec.set_timing(True)
    with pytest.raises(mp3_amd.MP3DError):
        dec.resample_time_us()  # no packed call yet
    run_whole(batch, (48000, 2), dec=dec)
    assert dec.resample_time_us() > 0.0
