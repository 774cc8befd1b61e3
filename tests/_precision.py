"""The float32 sink's precision contract: decoded float32
samples against the double oracle, in units of float32 rounding.

    e_peak   = max over frames f of max|got - ref| / (2^-24 A_f), A_f the
               reference's peak, all channels, over frame f and the frames
               within REACH = 1152 samples of it on either side
    e_rms    = rms(got - ref) / rms(ref) / 2^-24 over the stream
    e_silent = max|got| over the frames with A_f = 0: must be exactly 0

K_PEAK and K_RMS are 4 x what the float32 build of the oracle itself
(liboracle_f32.so: the same decoder, every operation in float32) reaches
against the double build over exactly the cases below, measured on the CPU
(tests/test_precision_host.py asserts it at K / 4).  The factor 4 covers the
kernel's other summation order (MFMA, factored IMDCT), a band scale built
from two rounded factors and a cube root good to 2 ulp: each worth a few eps.
The constants never come from what the GPU returns.

Why A_f looks both ways.  A granule's spectra land in the output of that
granule and of the two after it (IMDCT overlap: 576 samples, synthesis FIFO:
480 more), so a frame's rounding error scales with the spectra of two granules
back (their tail is still in the FIFO) and, at an onset, with spectra whose
energy shows only in the next two granules: the frame's own samples are small
there because two large IMDCT halves cancel.  With A_f over frames f and
f - 1 alone the float32 oracle itself reads 207 on keypress_128k_js (frame 0:
peak 1.7e-4 before a frame at 0.59) against 9.8 on everything else; 1152
samples are one MPEG-1 frame and two LSF frames.
"""
import ctypes

import numpy as np

import _gen
import _golden
import _oracle

EPS = 2.0 ** -24

# Measured maxima (e_peak, e_rms), float32 oracle against double oracle, per
# class of the cases below (16 streams x 10 frames each, the committed streams
# whole):
#   MPEG-1 long blocks (L/R, mono, M/S, M/S 320k, M/S + IS, IS)   7.17  3.36
#   MPEG-1 short / mixed heavy                                    7.27  3.06
#   C5 at 44.1 / 48 / 32 kHz                                      9.81  3.12
#   LSF 22.05 / 24 / 16 / 11.025 / 8 kHz                          6.91  3.30
#   level: M/S and M/S + IS at -40, -80, +40                      6.63  3.17
#   committed streams (keypress, c5_ms_is_mixed, lsf_scale_22k)   9.67  3.13
# The largest, rounded up to two digits, are 9.9 and 3.4.
K_PEAK = 4 * 9.9
K_RMS = 4 * 3.4

# The oracle (in double) and the kernel (in float32) both drop a requantised
# line below this magnitude; a reference line this close to it could fall on
# either side, so no case may hold one (tests/test_precision_host.py).
FLUSH = 0.5 * 1.759 * 2.0 ** -28
FLUSH_GUARD = 2.0 ** -20

N_STREAMS, N_FRAMES = 16, 10

_LONG = dict(_gen.C3, short_pct=0, mixed_pct=0)  # long blocks only
_MS = dict(_LONG, mode=1, mode_ext=2, crc_pct=0)
_MSIS = dict(_LONG, mode=1, mode_ext=3, crc_pct=0)
_LSF = {  # tests/golden/make_lsf_golden.py CASES
    3: dict(sr_idx=3, mode=1, mode_ext=-1, short_pct=30, mixed_pct=40),
    4: dict(sr_idx=4, mode=1, mode_ext=1, short_pct=20, mixed_pct=30),
    5: dict(sr_idx=5, mode=3, short_pct=25, mixed_pct=30, crc_pct=100),
    6: dict(sr_idx=6, mode=1, mode_ext=3, short_pct=25, mixed_pct=30),
    8: dict(sr_idx=8, mode=1, mode_ext=-1, short_pct=30, mixed_pct=40),
}

# name -> (generator settings, seed base, global_gain shift); stream s of a
# batch has seed base + s
CASES = {
    "lr_long": (dict(_LONG, mode=0, mode_ext=0), 12_100_001, 0),      # fused requantiser
    "mono_long": (dict(_LONG, mode=3, mode_ext=0), 12_100_101, 0),
    "ms_long": (_MS, 12_100_201, 0),                                   # all-long path
    "ms_long_320k": (dict(_MS, bitrate_idx=14, fill_pct=100), 10_302_962, 0),  # escapes: pow43_big
    "msis_long": (_MSIS, 12_100_401, 0),
    "is_long": (dict(_LONG, mode=1, mode_ext=1), 12_100_501, 0),
    "short_mixed": (dict(_gen.C3, short_pct=60, mixed_pct=30), 12_100_601, 0),
    "c5_44k": (dict(_gen.C5, sr_idx=0), 12_100_701, 0),
    "c5_48k": (dict(_gen.C5, sr_idx=1), 12_100_801, 0),
    "c5_32k": (dict(_gen.C5, sr_idx=2), 12_100_901, 0),
    "lsf_22k_js": (dict(_gen.C5, **_LSF[3]), 12_101_001, 0),
    "lsf_24k_is": (dict(_gen.C5, **_LSF[4]), 12_101_101, 0),
    "lsf_16k_mono_crc": (dict(_gen.C5, **_LSF[5]), 12_101_201, 0),
    "lsf_11k_ms_is": (dict(_gen.C5, **_LSF[6]), 12_101_301, 0),
    "lsf_8k_js": (dict(_gen.C5, **_LSF[8]), 12_101_401, 0),
    "ms_long_m40": (_MS, 12_100_201, -40),
    "ms_long_m80": (_MS, 12_100_201, -80),
    "ms_long_p40": (_MS, 12_100_201, +40),
    "msis_long_m40": (_MSIS, 12_100_401, -40),
    "msis_long_m80": (_MSIS, 12_100_401, -80),
    "msis_long_p40": (_MSIS, 12_100_401, +40),
}
# shifted by -160 every line requantises below FLUSH: all zeros, bit for bit
SILENT_CASES = {"ms_long_m160": (_MS, 12_100_201, -160), "msis_long_m160": (_MSIS, 12_100_401, -160)}
# committed streams (tests/golden/), against the double oracle and not their int16 PCM
GOLDEN_CASES = ["keypress_128k_js", "c5_ms_is_mixed", "lsf_scale_22k_js"]
# one stream through the per-frame decoder
PER_FRAME_CASE = ("c5_44k", 3)

_batches = {}


def batch(name):
    """(buf, offsets, sizes) of a generated case: read-only, made once"""
    if name not in _batches:
        cfg, seed, shift = {**CASES, **SILENT_CASES}[name]
        buf, offs, sizes = _gen.batch(cfg, seed, N_STREAMS, N_FRAMES, threads=4)
        if shift:
            buf = buf.copy()
            for o, n in zip(offs, sizes):
                o, n = int(o), int(n)
                buf[o:o + n] = np.frombuffer(shift_global_gain(bytes(buf[o:o + n]), shift), np.uint8)
        for a in (buf, offs, sizes):
            a.setflags(write=False)
        _batches[name] = (buf, offs, sizes)
    return _batches[name]


def streams(name):
    buf, offs, sizes = batch(name)
    return [bytes(buf[int(o):int(o) + int(n)]) for o, n in zip(offs, sizes)]


_HDR_INTS = 14  # orc_hdr


def oracle_frames(data, lib="liboracle.so"):
    """Yield (decoder, samples [ch, n] float64, frame info) per audio frame, as
    orc_decode_stream walks a stream (ID3v2 and a leading Xing/Info frame
    skipped, a cut last frame padded with zeros, dropped frames left out) but
    through orc_decode_frame_f64, which does not round to float32."""
    L = _oracle.lib(lib)
    dec = _oracle.Decoder(lib_name=lib)
    hdr = (ctypes.c_int * _HDR_INTS)()
    pos, first = L.orc_skip_id3v2(data, len(data)), True
    while pos + 4 <= len(data):
        fb = L.orc_parse_header(data[pos:pos + 4], hdr)
        if fb < 0:
            pos += 1
            continue
        frame = data[pos:pos + fb]
        if len(frame) < fb:
            crc_bytes, side_bytes = hdr[11], hdr[10]
            if len(frame) < 4 + crc_bytes + side_bytes:
                break
            frame = frame + bytes(fb - len(frame))
        elif first and L.orc_is_info_frame(frame, len(frame)):
            pos, first = pos + fb, False
            continue
        pos, first = pos + fb, False
        r, pcm, info = dec.decode_frame_f64(frame)
        if r > 0:
            yield dec, pcm[:, :r].copy(), info


def oracle_f64(data, lib="liboracle.so"):
    """float64 [F, ch, samples]: 1152 samples per MPEG-1 frame, 576 per LSF frame"""
    rows = [pcm for _, pcm, _ in oracle_frames(data, lib)]
    return np.stack(rows) if rows else np.zeros((0, 0, 0))


def frames_of(planar, ref):
    """planar [ch, F * samples] (mp3_amd.pcm_to_planar) as ref's [F, ch, samples]"""
    F, ch, n = ref.shape
    assert planar.shape == (ch, F * n), (planar.shape, ref.shape)
    return planar.reshape(ch, F, n).transpose(1, 0, 2)


REACH = 1152  # samples: two granules, what the overlap and the FIFO span together


def metric(got, ref):
    """(e_peak, e_rms, e_silent) of got against ref, both [F, ch, samples]"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and ref.ndim == 3 and ref.size, (got.shape, ref.shape)
    F, k = len(ref), REACH // ref.shape[2]
    peak = np.concatenate([np.zeros(k), np.abs(ref).max(axis=(1, 2)), np.zeros(k)])
    A = np.max([peak[i:i + F] for i in range(2 * k + 1)], axis=0)
    err = np.abs(got - ref).max(axis=(1, 2))
    live = A > 0
    e_peak = float((err[live] / (EPS * A[live])).max()) if live.any() else 0.0
    rms_ref = np.sqrt(np.mean(ref ** 2))
    e_rms = float(np.sqrt(np.mean((got - ref) ** 2)) / rms_ref / EPS) if rms_ref > 0 else 0.0
    e_silent = float(np.abs(got[~live]).max()) if (~live).any() else 0.0
    return e_peak, e_rms, e_silent


def shift_global_gain(data, delta):
    """The MPEG-1, CRC-less stream `data` (frames back to back) with `delta`
    added to the 8-bit global_gain of every unit of every frame, clamped to
    0 .. 255; every other bit as it was."""
    out = bytearray(data)
    pos = 0
    while pos + 4 <= len(out):
        b1, b2, b3 = out[pos + 1], out[pos + 2], out[pos + 3]
        assert out[pos] == 0xFF and (b1 & 0xFE) == 0xFA and (b1 & 1), "MPEG-1 Layer III without CRC only"
        kbps = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320][b2 >> 4]
        hz = [44100, 48000, 32000][(b2 >> 2) & 3]
        nch = 1 if (b3 >> 6) == 3 else 2
        for u in range(2 * nch):
            bit = 8 * (pos + 4) + 9 + (5 if nch == 1 else 3) + 4 * nch + 59 * u + 21
            v = 0
            for k in range(8):
                v = (v << 1) | ((out[(bit + k) >> 3] >> (7 - ((bit + k) & 7))) & 1)
            v = min(max(v + delta, 0), 255)
            for k in range(8):
                byte, mask = (bit + k) >> 3, 0x80 >> ((bit + k) & 7)
                out[byte] = (out[byte] | mask) if (v >> (7 - k)) & 1 else (out[byte] & ~mask & 0xFF)
        pos += 144000 * kbps // hz + ((b2 >> 1) & 1)
    return bytes(out)


def golden_stream(name):
    return _golden.case(name)[0]
