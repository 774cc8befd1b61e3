"""Anchors of the float32 precision contract (tests/_precision.py), on the CPU:
the float32 build of the oracle stays within a quarter of K_PEAK / K_RMS of
the double build on every case that tests/test_gpu_f32_precision.py decodes
on the GPU; the global_gain shifter touches that field alone; no case holds
a line at the flush threshold; and the bound catches a 1/sqrt(2) written as
0.7071 and a |is|^(4/3) off by 2e-5."""

import numpy as np
import pytest

import _oracle
import _precision as P
import _sideinfo
import _tables

HZ = [44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000]
GENERATED = list(P.CASES) + list(P.SILENT_CASES)


def _streams(name):
    return [P.golden_stream(name)] if name in P.GOLDEN_CASES else P.streams(name)


@pytest.mark.parametrize("name", GENERATED + P.GOLDEN_CASES)
def test_f32_oracle_within_a_quarter_of_the_bound(name):
    worst = [0.0, 0.0]
    for s, data in enumerate(_streams(name)):
        ref = P.oracle_f64(data)
        got = P.oracle_f64(data, "liboracle_f32.so")
        assert ref.shape == got.shape and ref.shape[0] >= (1 if name in P.GOLDEN_CASES else P.N_FRAMES), (name, s)
        e_peak, e_rms, e_silent = P.metric(got, ref)
        worst = [max(worst[0], e_peak), max(worst[1], e_rms)]
        assert e_silent == 0, (name, s)
        if name in P.SILENT_CASES:
            assert not ref.any() and not got.any(), (name, s)
        else:
            assert ref.any(), (name, s)
    print("%s: e_peak %.2f e_rms %.2f" % (name, *worst))
    assert worst[0] <= P.K_PEAK / 4 and worst[1] <= P.K_RMS / 4, (name, worst)


def test_metric_units():
    ref = np.zeros((5, 2, 1152))
    ref[1, 0, 2] = 0.5
    got = ref.copy()
    got[1, 1, 0] += 3 * P.EPS * 0.5   # 3 eps of frame 1's peak
    got[2, 0, 0] += 5 * P.EPS * 0.5   # frames 0 and 2 are silent, within reach of frame 1's peak
    got[0, 0, 9] -= 4 * P.EPS * 0.5
    e_peak, e_rms, e_silent = P.metric(got, ref)
    assert e_peak == 5.0 and e_silent == 0.0
    assert e_rms == pytest.approx(np.sqrt(50.0))  # sqrt(9 + 25 + 16) eps 0.5 over rms(ref) = 0.5, the 1 / N cancelling
    got[3, 0, 0] = 1e-30                # frames 3 and 4 have no reference peak within reach
    assert P.metric(got, ref) == (e_peak, pytest.approx(e_rms), 1e-30)
    lsf = np.zeros((5, 1, 576))
    lsf[0, 0, 0] = 1.0                  # 1152 samples are two LSF frames
    assert P.metric(lsf + np.eye(5)[3][:, None, None] * P.EPS, lsf) == (0.0, pytest.approx(np.sqrt(1.0 * 576)), P.EPS)
    assert P.metric(lsf + np.eye(5)[2][:, None, None] * P.EPS, lsf)[::2] == (1.0, 0.0)


def test_shifter_identity():
    for name in ("ms_long", "msis_long", "mono_long"):
        for data in P.streams(name)[:4]:
            assert P.shift_global_gain(data, 0) == data


@pytest.mark.parametrize("name,delta", [("ms_long", -40), ("msis_long", 40), ("mono_long", -80), ("ms_long", -160)])
def test_shifter_scope(name, delta):
    for data in P.streams(name)[:4]:
        out = P.shift_global_gain(data, delta)
        assert len(out) == len(data)
        fa, fb = list(_sideinfo.frames(data)), list(_sideinfo.frames(out))
        assert fa == fb and len(fa) == P.N_FRAMES
        clamped = 0
        for off, h in fa:
            a, b = _sideinfo.side_info(data, off, h), _sideinfo.side_info(out, off, h)
            for ua, ub in zip(sum(a["units"], []), sum(b["units"], [])):
                want = min(max(ua["global_gain"] + delta, 0), 255)
                clamped += want != ua["global_gain"] + delta
                assert ub["global_gain"] == want
                ua["global_gain"] = want
            assert a == b  # every other field
            side_end = off + 4 + (17 if h["mode"] == 3 else 32)
            assert out[off:off + 4] == data[off:off + 4]
            assert out[side_end:off + h["frame_bytes"]] == data[side_end:off + h["frame_bytes"]]  # main data
        assert clamped == 0 or abs(delta) >= 80


def _requant_pre_stereo(t, taps, hz, nch):
    """|xr| of every line as the requantiser makes it, before the flush and
    before joint stereo, from the oracle's is / scalefactor / side-info taps:
    |is|^(4/3) 2^(q / 4) (ISO 2.4.3.4), in double."""
    is_, sf, _, side = taps
    sr_idx = HZ.index(hz)
    lsf = sr_idx >= 3
    out = np.zeros((2, 2, 576))
    for gr in range(1 if lsf else 2):
        for ch in range(nch):
            o = side[gr, ch]
            gain, shift = int(o[2]) - 210, int(o[13]) + 1
            short = o[4] and o[5] == 2
            long_end = ((6 if lsf else 8) if o[6] else 0) if short else 22
            short_start = (3 if o[6] else 0) if short else 13
            q, j = [], 0
            for i in range(long_end):
                pre = int(t["MP3D_PRETAB"][i]) if o[12] else 0
                q += [gain - ((int(sf[gr, ch, j]) + pre) << shift)] * int(t["MP3D_SFB_LONG_WIDTH"][sr_idx][i])
                j += 1
            if short and o[6]:
                j = 8
            for i in range(short_start, 13 if short else 0):
                for w in range(3):
                    q += [gain - (int(o[17 + w]) << 3) - (int(sf[gr, ch, j]) << shift)] * int(t["MP3D_SFB_SHORT_WIDTH"][sr_idx][i])
                    j += 1
            assert len(q) == 576, len(q)
            out[gr, ch] = np.abs(is_[gr, ch].astype(np.float64)) ** (4.0 / 3.0) * 2.0 ** (0.25 * np.array(q))
    return out


def test_requant_restatement_matches_the_oracle_taps():
    """the helper above against the oracle's own xr, where no joint stereo
    mixes the channels (L/R, mono, and a short / mixed LSF mono case)"""
    t = _tables.load()
    for name in ("lr_long", "mono_long", "lsf_16k_mono_crc"):
        n = 0
        for dec, pcm, info in P.oracle_frames(P.streams(name)[0]):
            taps = dec.taps()
            x = _requant_pre_stereo(t, taps, info.hz, pcm.shape[0])
            x[x < P.FLUSH] = 0
            want = np.abs(taps[2].astype(np.float64))
            assert np.allclose(x, want, rtol=2.0 ** -22, atol=0), name
            n += int((want != 0).sum())
        assert n > 1000, (name, n)


@pytest.mark.parametrize("name", GENERATED + P.GOLDEN_CASES)
def test_no_line_at_the_flush_threshold(name):
    """The oracle flushes in double and the kernel in float32: a line within
    2^-20 of the threshold could go either way, so the cases hold none.  A
    seed that fails here is replaced, never masked."""
    t = _tables.load()
    lo, hi = P.FLUSH * (1 - P.FLUSH_GUARD), P.FLUSH * (1 + P.FLUSH_GUARD)
    lines = 0
    for s, data in enumerate(_streams(name)):
        for f, (dec, pcm, info) in enumerate(P.oracle_frames(data)):
            x = _requant_pre_stereo(t, dec.taps(), info.hz, pcm.shape[0])
            near = (x > lo) & (x < hi)
            assert not near.any(), (name, s, f, x[near])
            lines += int((x != 0).sum())
    assert lines > 0


def _xr_of(data):
    """the double oracle's xr taps [F, gr, ch, 576], its is taps and the block
    types, of an MPEG-1 stereo stream"""
    xr, is_, bt, mx = [], [], [], []
    for dec, _, _ in P.oracle_frames(data):
        i, _, x, side = dec.taps()
        xr.append(x)
        is_.append(i)
        bt.append(np.where(side[:, :, 4] != 0, side[:, :, 5], 0))
        mx.append(side[:, :, 6])
    return np.array(xr, np.float64), np.array(is_), np.array(bt, np.uint8), np.array(mx, np.uint8)


def _synth(xr, bt, mx):
    """orc_synth_only's float output as [F, ch, 1152]"""
    L = _oracle.lib()
    F, nch = xr.shape[0], xr.shape[2]
    x32 = np.ascontiguousarray(xr, np.float32)
    out = np.zeros((F, 1152, nch), np.float32)
    d = L.orc_create()
    L.orc_synth_only(d, x32.ctypes.data, bt.ctypes.data, mx.ctypes.data, F, nch, 0, None, out.ctypes.data)
    L.orc_destroy(d)
    return out.transpose(0, 2, 1)


def test_the_bound_has_teeth():
    """Two of the defects the bound is there to catch, seeded into the spectra
    of an M/S stream (no defective decoder is committed): both land beyond
    K_PEAK and K_RMS, though neither moves a sample by an int16 LSB."""
    data = P.streams("ms_long")[0]
    xr, is_, bt, mx = _xr_of(data)
    assert xr.shape == (P.N_FRAMES, 2, 2, 576) and not bt.any()
    clean = _synth(xr, bt, mx)
    assert np.abs(clean).max() > 0.1
    # (a) 1 / sqrt(2) of M/S written as 0.7071
    a = _synth(xr * (0.7071 * np.sqrt(2.0)), bt, mx)
    # (b) |is|^(4/3) off by 2e-5 for |is| >= 16, in the mid and side lines that the taps' L / R came from
    m, s = (xr[:, :, 0] + xr[:, :, 1]) / np.sqrt(2.0), (xr[:, :, 0] - xr[:, :, 1]) / np.sqrt(2.0)
    m = m * np.where(np.abs(is_[:, :, 0].astype(np.int32)) >= 16, 1 + 2e-5, 1.0)
    s = s * np.where(np.abs(is_[:, :, 1].astype(np.int32)) >= 16, 1 + 2e-5, 1.0)
    assert (np.abs(is_.astype(np.int32)) >= 16).any()
    b = _synth(np.stack([(m + s) / np.sqrt(2.0), (m - s) / np.sqrt(2.0)], axis=2), bt, mx)
    for what, got in (("0.7071", a), ("pow43", b)):
        e_peak, e_rms, e_silent = P.metric(got, clean)
        print("%s: e_peak %.1f e_rms %.1f max abs %.2e" % (what, e_peak, e_rms, np.abs(got - clean).max()))
        assert e_peak > P.K_PEAK and e_rms > P.K_RMS and e_silent == 0, (what, e_peak, e_rms)
        assert np.abs(got.astype(np.float64) - clean).max() < 2.0 ** -15  # invisible to the 1 LSB tolerance
