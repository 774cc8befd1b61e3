"""GPU: every (input rate, output rate) pair of the resampler through both
packed sinks -- 9 x 9 rates x {1, 2} output channels -- and k_rs_plan on more
than one block.

The batch is the nine 16-frame goldens, one per input rate, and an empty
stream.  rs_build (mp3d_sinks.cpp) never lets a tile span more than
MP3D_RS_SPAN - T - 2 <= 4 046 input samples, so 16 x 576 = 9 216 inputs are at
least three tiles of k_rs_filter for every pair: sixteen frames is the smallest
stream that runs first, inner and last tiles everywhere.  Each pair has its
own L, M, T, tile and S: 44.1 -> 8 kHz is M = 441 with T = 266 (T mod 4 = 2,
the scalar tail of the general path), 11.025 -> 32 kHz the 1 280-phase table,
48 -> 8 kHz fills 287 of the 288 history slots.

Expected values, as everywhere in tests/test_gpu_packed.py whose helpers
these tests use: the decoder's own plain float32 rows of a fresh handle,
channel mapped in float32, filtered in float64 with the taps of
resample_filter; the bound is that file's (T + 2) * 2^-24 * S * A.  The long
sink is compared with the batched sink bit for bit (test_gpu_long_packed.py's
long_run / packed_run), which ties it to the same reference.
"""
import numpy as np
import pytest

import _golden
import mp3_amd
import test_gpu_long_packed as LP
import test_gpu_packed as PK
from test_gpu_packed_window import Batch

pytestmark = pytest.mark.gpu

GOLD = ["c3_s0", "c5_mono_48k_crc", "c5_dual_32k_vbr", "lsf_22k_js", "lsf_24k_is", "lsf_16k_mono_crc",
        "lsf_11k_ms_is", "lsf_12k_stereo", "lsf_8k_js"]
GOLD_HZ = [44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000]
FORMATS = [(hz, ch) for hz in mp3_amd.RATES for ch in (1, 2)]
WIDTH = 300  # slots of the wide run: two blocks of k_rs_plan


@pytest.fixture(scope="module")
def batch():
    b = Batch(GOLD + ["empty"], [_golden.case(nm)[0] for nm in GOLD] + [b""])
    assert b.F == 16
    return b


@pytest.fixture(scope="module")
def plain(batch):
    rows, infos = PK.make_plain(batch)
    for s, hz in enumerate(GOLD_HZ):  # one stream per input rate, sixteen frames of audio each
        assert (infos[s]["samples"] > 0).all() and (infos[s]["hz"] == hz).all(), batch.names[s]
    assert sorted(GOLD_HZ) == sorted(mp3_amd.RATES)
    return rows, infos


@pytest.fixture(scope="module")
def expected(batch, plain):
    """Computed once."""
    return PK.make_expected(batch, plain, FORMATS)


# ---- A. the batched sink -----------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_values_and_counts(batch, expected, fmt):
    out, counts, _ = PK.run_whole(batch, fmt)
    PK.check_values(batch, expected, fmt, out, counts)
    for s in range(9):  # (check_values takes the counts from the reference: ceil(N L / M) here)
        n = 16 * (1152 if GOLD_HZ[s] >= 32000 else 576)
        L, M = PK.filt(GOLD_HZ[s], fmt[0])[:2]
        assert counts[s] == -(-n * L // M) > 0, (fmt, batch.names[s])
        T = PK.filt(GOLD_HZ[s], fmt[0])[2].shape[1]
        if T > 1:
            assert n > 2 * (4096 - T - 2)  # at least three tiles


def test_bypass_is_a_copy(batch, plain):
    rows, infos = plain
    seen = 0
    for fmt in FORMATS:
        out, counts, _ = PK.run_whole(batch, fmt)
        for s in range(batch.n):
            hz, x = PK.mapped_input(rows[s], infos[s], fmt[1])
            chans = {int(c) for c, k in zip(infos[s]["channels"], infos[s]["samples"]) if k}
            if hz != fmt[0] or chans != {fmt[1]}:
                continue
            seen += 1
            assert counts[s] == x.shape[0]
            assert np.array_equal(out[s, : counts[s]].view(np.uint32), x.view(np.uint32)), (fmt, batch.names[s])
    print("bypass hits: %d" % seen)
    assert seen >= 9


@pytest.mark.parametrize("fmt", FORMATS)
def test_chunking_is_bit_identical(batch, plain, fmt):
    """One call of 16 frames against sixteen calls of one frame, the flush on
    the last: the same bits, and per call the emit rule on the inputs so far."""
    rows, infos = plain
    whole, _ = PK.run_chunks(batch, fmt, [16])
    single, per_call = PK.run_chunks(batch, fmt, [1] * 16)
    for s in range(batch.n):
        assert np.array_equal(single[s].view(np.uint32), whole[s].view(np.uint32)), (fmt, batch.names[s])
        assert len(whole[s]) > 0 or batch.names[s] == "empty"
    for s in range(9):
        L, M, taps, pre, post = PK.filt(GOLD_HZ[s], fmt[0])
        seen = done = 0
        for i in range(16):
            seen += int(infos[s]["samples"][i])
            total = -(-seen * L // M) if i == 15 else PK.emitted(seen, L, M, post)
            assert per_call[i][s] == total - done, (fmt, batch.names[s], i)
            done = total
    assert all(c[batch.names.index("empty")] == 0 for c in per_call)


@pytest.mark.parametrize("fmt", FORMATS)
def test_int16_sink(batch, fmt):
    f, cf, _ = PK.run_whole(batch, fmt, f32=True)
    q, cq, _ = PK.run_whole(batch, fmt, f32=False)
    assert np.array_equal(cf, cq)
    for s in range(batch.n):
        assert np.array_equal(q[s, : cq[s]], _golden.to_int16(f[s, : cf[s]])), batch.names[s]
        assert (q[s, cq[s]:] == -1234).all()


def test_int16_clamps_at_both_rails(batch):
    """test_int16_sink proves the clamp only if some float32 output leaves the
    int16 range at each end: counted over the whole matrix, and at each rail
    the int16 sink holds the rail where the float32 sink is past it."""
    hi = lo = 0
    for fmt in FORMATS:
        f, cf, _ = PK.run_whole(batch, fmt, f32=True)
        q, cq, _ = PK.run_whole(batch, fmt, f32=False)
        for s in range(batch.n):
            v = f[s, : cf[s]].astype(np.float64) * 32768.0
            over, under = v >= 32767.5, v < -32768.0
            hi += int(over.sum())
            lo += int(under.sum())
            assert (q[s, : cq[s]][over] == 32767).all() and (q[s, : cq[s]][under] == -32768).all(), (fmt, s)
    print("clamped samples over the matrix: %d at +32767, %d at -32768" % (hi, lo))
    assert hi >= 1 and lo >= 1


@pytest.mark.parametrize("fmt", [(32000, 2), (8000, 1)])
def test_width(fmt):
    """300 slots, the nine streams round-robin: k_rs_plan's second block
    (stream index blockIdx.x * 256 + threadIdx.x).  (32000, 2) upsamples six
    of the input rates, (8000, 1) downsamples eight."""
    streams = [_golden.case(nm)[0] for nm in GOLD]
    nine = Batch(GOLD, streams)
    wide = Batch(["%s@%d" % (GOLD[s % 9], s) for s in range(WIDTH)], [streams[s % 9] for s in range(WIDTH)])
    assert wide.n == WIDTH > 256 and wide.F == nine.F == 16
    want, want_counts, _ = PK.run_whole(nine, fmt)
    got, counts, _ = PK.run_whole(wide, fmt)
    assert (want_counts > 0).all()
    for s in range(WIDTH):
        assert counts[s] == want_counts[s % 9], wide.names[s]
        assert np.array_equal(got[s].view(np.uint32), want[s % 9].view(np.uint32)), wide.names[s]  # pattern included


# ---- B. the long sink --------------------------------------------------------
@pytest.mark.parametrize("name,fmt", [(nm, (hz, 2 if (s + r) % 2 == 0 else 1)) for s, nm in enumerate(GOLD)
                                      for r, hz in enumerate(mp3_amd.RATES)])
def test_long_sink_equals_the_packed_sink(name, fmt):
    """Chunks of 12 frames (geometry (4, 3)): the second chunk's tiles read
    the carry.  long_run checks the pattern past the count."""
    data = _golden.case(name)[0]
    got, in_hz, _ = LP.long_run(data, fmt, gapless=False, geom=(4, 3))
    assert in_hz == GOLD_HZ[GOLD.index(name)]
    L, M = PK.filt(in_hz, fmt[0])[:2]
    assert len(got) == -(-16 * (1152 if in_hz >= 32000 else 576) * L // M)
    LP.same_bits(got, LP.packed_run(data, fmt), (name, fmt))
