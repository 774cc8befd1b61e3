"""The host-only half of the log-mel feature sink (include/mp3d.h "log-mel
feature sink"; no GPU needed): the Slaney filterbank against a float64
restatement of the header's formula, the stride bound against the emit rule
by brute force, argument errors and the exports."""
import ctypes

import numpy as np
import pytest

import mp3_amd

NEW = ["mp3d_batch_decode_features", "mp3d_batch_feature_time", "mp3d_batch_features", "mp3d_batch_set_features",
       "mp3d_feat_max_frames", "mp3d_mel_filterbank"]


def mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + np.log(np.maximum(f, 1.0) / 1000.0) * 27.0 / np.log(6.4))


def hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp((m - 15.0) * np.log(6.4) / 27.0))


def filterbank64(n_mels):
    """F[j][k] of the header in float64."""
    c = hz(np.arange(n_mels + 2) * float(mel(8000.0)) / (n_mels + 1))
    f = 40.0 * np.arange(201)
    up = (f[None, :] - c[:-2, None]) / (c[1:-1] - c[:-2])[:, None]
    down = (c[2:, None] - f[None, :]) / (c[2:] - c[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(up, down)) * (2.0 / (c[2:] - c[:-2]))[:, None]


def emitted(n):
    n = np.asarray(n, np.int64)
    return np.where(n >= 200, (n - 200) // 160 + 1, 0)


@pytest.mark.parametrize("n_mels", [40, 80, 128])
def test_filterbank_is_the_formula(n_mels):
    fb = mp3_amd.mel_filterbank(n_mels)
    assert fb.dtype == np.float32 and fb.shape == (n_mels, 201)
    want = filterbank64(n_mels).astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(fb.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert (fb >= 0).all()
    widths = []
    for j in range(n_mels):
        nz = np.flatnonzero(fb[j])
        assert nz.size >= 1 and nz[-1] - nz[0] + 1 == nz.size, j  # one contiguous support
        widths.append(nz.size)
    assert ((fb > 0).sum(axis=0) <= 2).all()  # no bin lies in more than two filters
    print("n_mels %d: supports of %d .. %d bins" % (n_mels, min(widths), max(widths)))


def test_filterbank_argument_errors():
    L = mp3_amd.lib()
    buf = np.zeros(80 * 201, np.float32)
    assert L.mp3d_mel_filterbank(0, None, 0) == -1
    assert L.mp3d_mel_filterbank(129, None, 0) == -1
    assert L.mp3d_mel_filterbank(-1, None, 0) == -1
    assert L.mp3d_mel_filterbank(80, None, 0) == 80 * 201
    assert L.mp3d_mel_filterbank(80, buf.ctypes.data, 80 * 201 - 1) == -1  # short cap
    assert not buf.any()
    assert L.mp3d_mel_filterbank(80, buf.ctypes.data, 80 * 201) == 80 * 201
    assert L.mp3d_mel_filterbank(1, buf.ctypes.data, 201) == 201 and L.mp3d_mel_filterbank(128, None, 0) == 128 * 201
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        mp3_amd.mel_filterbank(129)


@pytest.mark.parametrize("frames,min_hz", [(1, 8000), (1, 32000), (2, 8000), (3, 44100), (16, 48000)])
def test_feat_max_frames(frames, min_hz):
    S = mp3_amd.packed_max_samples(16000, frames, min_hz)
    bound = mp3_amd.feat_max_frames(frames, min_hz)
    assert S > 0 and bound == -(-(S + 200) // 160) + 1
    # whatever is pending, S new samples never emit more, flushed or not
    n0 = np.arange(401, dtype=np.int64)[:, None]
    s = np.arange(S + 1, dtype=np.int64)[None, :]
    plain = emitted(n0 + s) - emitted(n0)
    flushed = -(-(n0 + s) // 160) - emitted(n0)
    assert plain.max() <= bound and flushed.max() <= bound
    assert flushed.max() >= bound - 2  # (and the bound is not loose by more than the rounding)


def test_feat_max_frames_edges():
    assert mp3_amd.feat_max_frames(4) == mp3_amd.feat_max_frames(4, 8000)
    assert mp3_amd.lib().mp3d_feat_max_frames(4, 48001) == 0  # no input rate that high: S = 0
    assert mp3_amd.lib().mp3d_feat_max_frames(-1, 8000) == -1


def test_exports():
    names = sorted(mp3_amd.EXPORTS)
    for n in NEW:
        assert n in names, n
    L = mp3_amd.lib()
    for n in NEW:
        assert hasattr(L, n), n
    assert mp3_amd.FEAT_LOG10 == 1 and mp3_amd.MP3D_FEAT_LOG10 == 1
    assert L.mp3d_abi_version() == 5
    # a NULL handle is refused before anything touches a device
    assert L.mp3d_batch_set_features(None, 80, 1) == -1
    assert L.mp3d_batch_feature_time(None, ctypes.byref(ctypes.c_float())) == -1
