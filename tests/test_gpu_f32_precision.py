"""The float32 sink against the double oracle at float32 precision
(tests/_precision.py): every k_synth path, every LSF rate,
streams 60 and 120 dB below and 60 dB above the usual level, streams that
requantise to nothing, and committed real content.  Each stream of each case
must stay within K_PEAK float32 roundings of the local peak and K_RMS of the
stream's RMS, and be exactly zero where the reference is.  The bounds are 4 x
what a plain float32 evaluation of the same decoder reaches on these very
streams (tests/test_precision_host.py); the 1 LSB tolerance of the other
modules is about 100 times looser."""
import numpy as np
import pytest

import _precision as P
import mp3_amd

pytestmark = pytest.mark.gpu


def _decode(name):
    buf, offs, sizes = P.batch(name)
    pcm, infos = mp3_amd.BatchDecoder(P.N_STREAMS, P.N_FRAMES).decode(buf, offs, sizes, P.N_FRAMES, f32=True)
    assert pcm.dtype == np.float32
    return [mp3_amd.pcm_to_planar(pcm[s], infos[s]) for s in range(P.N_STREAMS)]


def _check(what, planar, data):
    ref = P.oracle_f64(data)
    e_peak, e_rms, e_silent = P.metric(P.frames_of(planar, ref), ref)
    print("%s: e_peak %.2f e_rms %.2f e_silent %g" % (what, e_peak, e_rms, e_silent))
    return (what, e_peak, e_rms, e_silent), ref


def _assert_all(rows):
    bad = [r for r in rows if not (r[1] <= P.K_PEAK and r[2] <= P.K_RMS and r[3] == 0)]
    assert not bad, bad


@pytest.mark.parametrize("name", list(P.CASES))
def test_generated_case(name):
    rows = []
    for s, (got, data) in enumerate(zip(_decode(name), P.streams(name))):
        row, ref = _check("%s[%d]" % (name, s), got, data)
        assert ref.shape[0] == P.N_FRAMES and ref.any()
        rows.append(row)
    _assert_all(rows)


def test_escapes_occur_in_the_320k_case():
    buf, offs, sizes = P.batch("ms_long_320k")
    rows, _ = mp3_amd.BatchDecoder(P.N_STREAMS, P.N_FRAMES).huffman_only(buf, offs, sizes, P.N_FRAMES)
    big = (np.abs(np.asarray(rows).astype(np.int32)) >= 256).reshape(P.N_STREAMS, -1).sum(axis=1)
    assert (big > 0).sum() >= P.N_STREAMS // 2 and big.sum() >= 20, big  # pow43_big runs


@pytest.mark.parametrize("name", list(P.SILENT_CASES))
def test_below_the_flush_threshold_is_silence(name):
    for s, (got, data) in enumerate(zip(_decode(name), P.streams(name))):
        ref = P.oracle_f64(data)
        assert got.shape == (2, P.N_FRAMES * 1152) and not ref.any()
        assert not got.view(np.uint32).any(), (name, s, np.abs(got).max())  # +0.0, bit for bit


@pytest.mark.parametrize("name", P.GOLDEN_CASES)
def test_committed_stream(name):
    data = P.golden_stream(name)
    ref = P.oracle_f64(data)
    nf = ref.shape[0] + 4
    pcm, infos = mp3_amd.BatchDecoder(1, nf).decode(np.frombuffer(data, np.uint8), [0], [len(data)], nf, f32=True)
    row, _ = _check(name, mp3_amd.pcm_to_planar(pcm[0], infos[0]), data)
    _assert_all([row])


def test_per_frame_decoder():
    name, s = P.PER_FRAME_CASE
    data = P.streams(name)[s]
    row, _ = _check("per-frame %s[%d]" % (name, s), mp3_amd.Decoder().decode_stream(data, f32=True), data)
    _assert_all([row])
