"""GPU: mp3d_batch_kernel_times, the core decode's chain of four events
(before demux, after demux, after Huffman, after synthesis) on the call's
stream: the three intervals nest inside a pair of events the caller records
around the call on the same stream; synth_only records the three front events
back to back; a handle whose timing is off refuses the query."""
import math

import numpy as np
import pytest
import torch

import _gen
import mp3_amd

pytestmark = pytest.mark.gpu

N, F = 4, 4
# Events on one stream are ordered, so demux + huffman + synth can exceed the
# caller's outer interval only by the rounding of four float32 millisecond
# differences.  Largest excess measured over 20 repetitions before the core
# path moved onto the shared call frame: -14.5 us (the sum, ~72 us, was below
# the outer interval, ~87 us, every time), so no slack is allowed.
SLACK_US = 0.0


def _timed_decode(dec, d_in, offs, sizes, pcm, infos, strm):
    """one decode on strm between two of the caller's events: (times, outer us)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(strm)
    dec.decode(d_in, offs, sizes, F, pcm=pcm, infos=infos, stream=strm.cuda_stream)
    e1.record(strm)
    e1.synchronize()
    return dec.kernel_times_us(), e0.elapsed_time(e1) * 1000.0


@pytest.fixture(scope="module")
def timed():
    buf, offs, sizes = _gen.batch(_gen.C3, 1501, N, F)
    dec = mp3_amd.BatchDecoder(N, F)
    d_in = torch.from_numpy(buf).cuda()
    pcm = torch.zeros((N, F, 2304), dtype=torch.int16, device="cuda")
    infos = torch.zeros((N, F, 6), dtype=torch.int32, device="cuda")
    strm = torch.cuda.Stream()
    dec.set_timing(True)
    return dec, d_in, offs, sizes, pcm, infos, strm


def test_kernel_times_nest_in_the_callers_events(timed):
    dec, d_in, offs, sizes, pcm, infos, strm = timed
    t, outer = _timed_decode(dec, d_in, offs, sizes, pcm, infos, strm)
    print("kernel_times_us", t, "outer_us", outer, "excess_us", sum(t.values()) - outer)
    assert all(math.isfinite(v) and v >= 0 for v in t.values()), t
    assert t["synth"] > 0, t
    assert t["demux"] + t["huffman"] + t["synth"] <= outer + SLACK_US, (t, outer)
    assert int((infos[:, :, 5] == 1152).sum()) == N * F  # (the timed call decoded)


def test_kernel_times_after_synth_only(timed):
    dec = timed[0]
    strm = timed[-1]
    rng = np.random.default_rng(1502)
    xr = torch.from_numpy((rng.standard_normal((N, F, 2, 2, 576)) * 0.01).astype(np.float32)).cuda()
    bt = torch.zeros((N, F, 2, 2), dtype=torch.uint8, device="cuda")
    mx = torch.zeros((N, F, 2, 2), dtype=torch.uint8, device="cuda")
    pcm = torch.zeros((N, F, 2304), dtype=torch.int16, device="cuda")
    dec.synth_only(xr, bt, mx, 2, 44100, pcm=pcm, stream=strm.cuda_stream)
    t = dec.kernel_times_us()
    print("kernel_times_us after synth_only", t)
    # the three front events are recorded back to back
    assert all(math.isfinite(v) for v in t.values()), t
    assert t["demux"] >= 0 and t["huffman"] >= 0, t
    assert t["synth"] > 0, t


def test_kernel_times_need_timing():
    buf, offs, sizes = _gen.batch(_gen.C3, 1501, N, F)
    dec = mp3_amd.BatchDecoder(N, F)
    dec.decode(buf, offs, sizes, F)
    with pytest.raises(mp3_amd.MP3DError) as e:
        dec.kernel_times_us()
    assert "mp3d error -1 " in str(e.value)
