"""The host-only half of the equaliser sink (include/mp3d.h "equaliser sink"; no
GPU needed): mp3d_eq_design against the long-double cookbook design of
tests/_eq.py, facts of the curves, argument errors, the exports; the
measurement behind the numerical contract's eps (the float64 time-parallel
restatement against a long-double sequential evaluation over the whole test
list) with its cap; and seeded defects in the restatement that the bound must
catch -- and one it does not see."""
import ctypes

import numpy as np
import pytest

import _eq
import mp3_amd

NEW = ["mp3d_eq_design", "mp3d_batch_set_eq", "mp3d_batch_eq", "mp3d_batch_decode_equalized", "mp3d_batch_eq_time"]
E_ARG = -1


def test_exports():
    L = mp3_amd.lib()
    for n in NEW:
        assert n in mp3_amd.EXPORTS and hasattr(L, n), n
    assert L.mp3d_abi_version() == 5  # additive: the ABI version stays
    assert mp3_amd.EQ_MAX_BANDS == _eq.MAX_BANDS
    assert (mp3_amd.EQ_PEAK, mp3_amd.EQ_LOW_SHELF, mp3_amd.EQ_HIGH_SHELF, mp3_amd.EQ_HIGH_PASS,
            mp3_amd.EQ_LOW_PASS) == (_eq.PEAK, _eq.LOW_SHELF, _eq.HIGH_SHELF, _eq.HIGH_PASS, _eq.LOW_PASS)
    assert mp3_amd.EQ_BAND_DT.itemsize == 32  # mp3d_eq_band: int, padding, three doubles


# ---- the design --------------------------------------------------------------------------
def ulps(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want))))


@pytest.mark.parametrize("hz", mp3_amd.RATES)
def test_design_is_the_cookbook_in_long_double(hz):
    for name in _eq.CURVES:
        bands, pre = _eq.curve(name, hz)
        got = mp3_amd.eq_design(hz, bands, pre)
        assert got.shape == (len(bands), 5) and got.dtype == np.float64
        assert ulps(got, _eq.design64(hz, bands, pre)) <= 1.0, (hz, name)
    # every type at the corners of the accepted ranges
    for typ in range(5):
        for f0 in (20.0, 0.45 * hz):
            for q in (0.1, 16.0):
                for g in (-24.0, 24.0):
                    b = [(typ, f0, g, q)]
                    assert ulps(mp3_amd.eq_design(hz, b, 24.0), _eq.design64(hz, b, 24.0)) <= 1.0, (hz, b)


@pytest.mark.parametrize("hz", mp3_amd.RATES)
def test_peaking_band_has_its_gain_at_f0(hz):
    for g in (-24.0, -12.0, 3.0, 12.0):
        for f0, q in ((20.0, 16.0), (1000.0, 1.41), (0.45 * hz, 0.1)):
            c = mp3_amd.eq_design(hz, [(_eq.PEAK, f0, g, q)])
            assert abs(float(_eq.response_db(c, f0, hz)) - g) <= 1e-9, (hz, g, f0, q)


def test_a_flat_peaking_curve_is_the_identity():
    for hz in mp3_amd.RATES:
        bands, pre = _eq.curve("flat", hz)
        c = mp3_amd.eq_design(hz, bands, pre)
        assert (c[:, 0] == 1.0).all() and (c[:, 1] == c[:, 3]).all() and (c[:, 2] == c[:, 4]).all()


def test_preamp_scales_stage_one_only():
    hz = 44100
    bands, _ = _eq.curve("five_types", hz)
    base, amp = mp3_amd.eq_design(hz, bands, 0.0), mp3_amd.eq_design(hz, bands, -6.0)
    assert (base[1:] == amp[1:]).all() and (base[0, 3:] == amp[0, 3:]).all()
    g = 10.0 ** (-6.0 / 20.0)
    assert np.allclose(amp[0, :3], base[0, :3] * g, rtol=4e-16, atol=0)
    assert ulps(amp, _eq.design64(hz, bands, -6.0)) <= 1.0


def test_design_argument_errors():
    L = mp3_amd.lib()
    ok = [(_eq.PEAK, 1000.0, 3.0, 1.0)]

    def rc(hz, bands, pre=0.0, cap=None, coef=True):
        arr = mp3_amd._eq_bands(bands)
        out = np.zeros(5 * max(1, arr.size))
        return L.mp3d_eq_design(hz, arr.ctypes.data if arr.size else None, arr.size, pre,
                                out.ctypes.data if coef else None, out.size if cap is None else cap)

    assert rc(48000, ok) == 5 and rc(48000, ok * 10) == 50
    assert rc(48000, ok, coef=False, cap=0) == 5  # the size only
    for hz in (0, 7999, 44000, 96000):
        assert rc(hz, ok) == E_ARG
    assert rc(48000, ok * 2, cap=9) == E_ARG and rc(48000, ok, cap=4) == E_ARG
    assert rc(48000, []) == E_ARG and rc(48000, ok * 11) == E_ARG
    nan = float("nan")
    for pre in (-24.01, 24.01, nan):
        assert rc(48000, ok, pre) == E_ARG
    for bad in [(-1, 1000.0, 0.0, 1.0), (5, 1000.0, 0.0, 1.0),
                (_eq.PEAK, 19.99, 0.0, 1.0), (_eq.PEAK, 0.45 * 48000 + 0.01, 0.0, 1.0), (_eq.PEAK, nan, 0.0, 1.0),
                (_eq.PEAK, 1000.0, -24.01, 1.0), (_eq.PEAK, 1000.0, 24.01, 1.0), (_eq.PEAK, 1000.0, nan, 1.0),
                (_eq.HIGH_PASS, 1000.0, 30.0, 1.0),
                (_eq.PEAK, 1000.0, 0.0, 0.0999), (_eq.PEAK, 1000.0, 0.0, 16.01), (_eq.PEAK, 1000.0, 0.0, nan)]:
        assert rc(48000, [bad]) == E_ARG, bad
        assert rc(48000, ok + [bad]) == E_ARG, bad
    # the frequency limit follows the rate
    assert rc(8000, [(_eq.PEAK, 3600.0, 0.0, 1.0)]) == 5 and rc(8000, [(_eq.PEAK, 3600.5, 0.0, 1.0)]) == E_ARG
    with pytest.raises(mp3_amd.MP3DError):
        mp3_amd.eq_design(48000, [])
    # a handle is needed for the rest: without one the calls fail, they do not crash
    assert L.mp3d_batch_set_eq(None, None, 0, 0.0) == E_ARG
    assert L.mp3d_batch_eq_time(None, None) == E_ARG


# ---- the definition's two evaluations agree with a plain loop ------------------------------
def test_seq_is_the_sample_loop():
    hz = 48000
    bands, pre = _eq.curve("five_types", hz)
    c = _eq.design64(hz, bands, pre)
    x = _eq.signal("noise", hz, 300, 2)
    want = np.zeros((300, 2))
    for ch in range(2):
        v = x[:, ch].astype(np.float64)
        for b0, b1, b2, a1, a2 in c:
            s1 = s2 = 0.0
            o = np.zeros(300)
            for i, t in enumerate(v.tolist()):
                y = b0 * t + s1
                s1 = b1 * t - a1 * y + s2
                s2 = b2 * t - a2 * y
                o[i] = y
            v = o
        want[:, ch] = v
    assert (_eq.seq(c, x) == want).all()


# ---- eps: measured, capped ------------------------------------------------------------------
def restated(hz, ch, name, defect=None, coef=None):
    """par64 over the ragged batch: [(n, y float64 [n, ch])] per stream"""
    if coef is None:
        bands, pre = _eq.curve(name, hz)
        coef = _eq.design64(hz, bands, pre)
    out = []
    for _, n, x in _eq.streams(hz, ch):
        out.append((n, _eq.par64(coef, x.T, defect).T))
    return out


def test_eps_is_four_times_the_measured_error_and_under_the_cap():
    assert _eq.EPS == 4 * _eq.EPS_MEASURED and _eq.EPS <= _eq.EPS_CAP == 2.0 ** -26
    worst = (0.0, None)
    for hz, ch in _eq.FORMATS:
        for name in _eq.CURVES:
            ref = _eq.reference(hz, ch, name, np.longdouble)
            for (sig, n, _), (_, y), (_, r) in zip(_eq.streams(hz, ch), restated(hz, ch, name), ref):
                if not n:
                    continue
                G = np.maximum.accumulate(np.abs(r), axis=0)
                err = np.abs(y.astype(np.longdouble) - r)
                assert (err[G == 0] == 0).all()
                e = float((err[G > 0] / G[G > 0]).max()) if (G > 0).any() else 0.0
                if e > worst[0]:
                    worst = (e, (hz, ch, name, sig, n))
    print("largest |par64 - longdouble| / G: %.3g at %s" % worst)
    assert worst[0] <= _eq.EPS_MEASURED
    assert worst[0] >= _eq.EPS_MEASURED / 4  # (the constant is the measurement, not a guess far above it)


def test_the_sequential_float64_form_is_inside_the_bound_too():
    """the reference of the GPU test against long double: a small part of eps"""
    for hz, ch in _eq.FORMATS[:1]:
        for name in _eq.CURVES:
            for (n, r64), (_, rld) in zip(_eq.reference(hz, ch, name), _eq.reference(hz, ch, name, np.longdouble)):
                assert _eq.excess(r64, rld.astype(np.float64), eps=_eq.EPS / 4) <= 1.0


# ---- seeded defects ----------------------------------------------------------------------------
HZ, CH = 48000, 2


def f32(y):
    return np.asarray(y, np.float32)


def worst_excess(got, hz, ch, name):
    """over the streams: the float32-rounded result against the float64 sequential reference"""
    return max(_eq.excess(f32(y), r) for (_, y), (_, r) in zip(got, _eq.reference(hz, ch, name)))


def test_the_restatement_passes_the_bound():
    for name in _eq.CURVES:
        assert worst_excess(restated(HZ, CH, name), HZ, CH, name) <= 1.0, name


@pytest.mark.parametrize("defect", ["f32_state", "shift", "no_carry"])
def test_the_bound_catches_a_defect_in_the_time_parallel_form(defect):
    for name in ("pole20", "graphic"):
        e = worst_excess(restated(HZ, CH, name, defect), HZ, CH, name)
        print(defect, name, "err / bound = %.3g" % e)
        assert e > 100.0, (defect, name, e)


def test_the_bound_catches_swapped_feedback_coefficients():
    for name in ("graphic", "five_types"):
        bands, pre = _eq.curve(name, HZ)
        c = _eq.design64(HZ, bands, pre)[:, [0, 1, 2, 4, 3]]
        with np.errstate(all="ignore"):
            e = worst_excess(restated(HZ, CH, name, coef=c), HZ, CH, name)
        assert e > 100.0, (name, e)


def test_what_the_bound_does_not_see_reversed_stage_order():
    """The sections commute: from a zero state their order shows only in the
    rounding, so a cascade run backwards is inside the bound.  (With no preamp:
    the curve's stage 1 carries it wherever it stands.)"""
    bands, pre = _eq.curve("five_types", HZ)
    assert pre == 0.0
    c = _eq.design64(HZ, bands, pre)[::-1].copy()
    got = restated(HZ, CH, "five_types", coef=c)
    e = worst_excess(got, HZ, CH, "five_types")
    print("reversed order: err / bound = %.3g" % e)
    assert e <= 1.0
    # and it is another computation: some sample differs in float64
    fwd = restated(HZ, CH, "five_types")
    assert any((a != b).any() for (_, a), (_, b) in zip(got, fwd))
