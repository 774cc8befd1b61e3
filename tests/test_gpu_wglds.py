"""GPU: the per-workgroup LDS poison build (mp3_amd/libmp3d_wglds.so,
-DMP3D_WG_LDS_POISON) against the product library, bit for bit.

In that build MP3D_LDS_ENTRY() (mp3d_device.h), the first statement of every
kernel, makes every workgroup fill its whole static LDS allocation with 0xFF
and meet at a barrier before anything else.  A kernel that reads static LDS
its own workgroup did not write then computes with all-ones words (NaN as
float, huge lengths) in EVERY workgroup, where the product build sees what
the previous workgroup on the CU left: its output differs from the product's,
or it fails, on every run.  Identical bytes on the cases below -- every
kernel of the library, several workgroups per CU -- mean no such read exists
on the paths they take.

test_probe is the positive control: the fill really covers the whole
allocation of every workgroup (the byte tail of a size that is no multiple of
4 included), whatever the CU's LDS held before.

Both builds live in one process: mp3_amd.library() selects the build for the
handles created inside it, and a handle keeps its build.  Handles are fresh in
every run, and MP3D_DEBUG_POISON is off: this is the product's condition."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _gen
import _golden
import mp3_amd
import test_gpu_packed as PK
import test_gpu_readahead as RA
from mp3_amd import _build

pytestmark = pytest.mark.gpu

WGLDS = _build.WGLDS_LIB
LSF = dict(_gen.C5, sr_idx=-2, short_pct=30, mixed_pct=40)


def _same(a, b, where=""):
    """Bit-for-bit equality of nested results (arrays by their bytes: a NaN
    equals the same NaN, -0.0 does not equal 0.0)."""
    if isinstance(a, (tuple, list)):
        assert type(a) is type(b) and len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (where, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, where
        xa, xb = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
        if not np.array_equal(xa, xb):
            first = int(np.flatnonzero(xa != xb)[0]) // a.dtype.itemsize
            raise AssertionError("%s: first differing element %s of shape %s" %
                                 (where, np.unravel_index(first, a.shape), a.shape))
    else:
        assert a == b, where


def _both(run):
    """run() under the product library and under the wglds build."""
    want = run()
    with mp3_amd.library(WGLDS):
        got = run()
    _same(got, want, run.__name__)
    return want


def _decode(buf, offs, sizes, n, F, f32=False, env=None):
    """One batch call on a fresh handle: (pcm, infos, state blobs, stream infos)."""
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        dec = mp3_amd.BatchDecoder(n, F)
        pcm, infos = dec.decode(buf, offs, sizes, F, f32=f32)
        return pcm, infos, dec.get_state(0, n), [bytes(x) for x in dec.stream_info(n)]
    finally:
        for k in env or {}:
            os.environ.pop(k, None)


def _mixed_family(F=6, n=24):
    b1, o1, s1 = _gen.batch(_gen.C5, 601, n, F)
    b2, o2, s2 = _gen.batch(LSF, 602, n, F)
    offs, sizes = np.empty(2 * n, np.uint64), np.empty(2 * n, np.uint32)
    offs[0::2], sizes[0::2] = o1, s1
    offs[1::2], sizes[1::2] = o2 + len(b1), s2
    return np.concatenate([b1, b2]), offs, sizes


def test_probe():
    """8 workgroups per CU, after 0x5A5A5A5A was left in the CUs' LDS: every
    byte of every workgroup's static LDS is 0xFF after the entry fill.  The
    product library has no probe."""
    product = ctypes.CDLL(str(_build.ROOT / "mp3_amd" / "libmp3d.so"))
    assert not hasattr(product, "mp3d_debug_wglds_probe")
    with mp3_amd.library(WGLDS) as L:
        W = L.mp3d_debug_wglds_probe(0, 0, None, 0)
        n = 8 * torch.cuda.get_device_properties(0).multi_processor_count
        out = np.zeros((n, W), np.uint32)
        nbytes = L.mp3d_debug_wglds_probe(0, n, out.ctypes.data, W)
    assert nbytes == 4667 and W == 1167, (nbytes, W)  # (k_wglds_probe: a size with a 3-byte tail)
    full = nbytes // 4
    print("probe: %d workgroups x %d B; words 0xFFFFFFFF: %d of %d; words 0x5A5A5A5A: %d" %
          (n, nbytes, int((out[:, :full] == 0xFFFFFFFF).sum()), n * full, int((out == 0x5A5A5A5A).sum())))
    assert (out[:, :full] == 0xFFFFFFFF).all()
    assert (out[:, full] == 0x00FFFFFF).all()  # the tail's 3 bytes; the byte past the allocation is not read
    assert not (out.view(np.uint8) == 0x5A).any()


def test_handles_keep_their_build():
    """A handle made inside library() calls that build after the block ends
    (decode, state, destroy), next to a handle of the current build."""
    buf, offs, sizes = _gen.batch(_gen.C3, 7, 3, 2)
    before = mp3_amd.lib()
    with mp3_amd.library(WGLDS) as L:
        assert mp3_amd.lib() is L and hasattr(L, "mp3d_debug_wglds_probe")
        a, d = mp3_amd.BatchDecoder(3, 2), mp3_amd.Decoder()
    assert mp3_amd.lib() is before
    b = mp3_amd.BatchDecoder(3, 2)
    assert a._L is L and d._L is L and b._L is before
    _same(a.decode(buf, offs, sizes, 2), b.decode(buf, offs, sizes, 2))
    _same(a.get_state(0, 3), b.get_state(0, 3))
    data = bytes(buf[offs[0]:offs[0] + sizes[0]])
    _same(d.decode_frame(data)[1], mp3_amd.Decoder().decode_frame(data)[1])
    for h in (a, b, d):
        h.close()


@pytest.mark.parametrize("f32", [False, True])
def test_ragged_mixed_batch(f32):
    n, F = 37, 5
    buf, offs, sizes = _gen.batch(_gen.C5, 501, n, F)

    def ragged():
        return _decode(buf, offs, sizes, n, F, f32)
    pcm, infos, _, _ = _both(ragged)
    assert (infos["samples"] > 0).all() and pcm.any()


@pytest.mark.parametrize("f32", [False, True])
def test_mixed_family_batch(f32):
    buf, offs, sizes = _mixed_family()

    def mixed():
        return _decode(buf, offs, sizes, 48, 6, f32)
    _, infos, _, _ = _both(mixed)
    assert set(np.unique(infos["samples"])) == {576, 1152}


def test_high_bitrate_staging():
    cfg = dict(_gen.C5)
    cfg.update(sr_idx=2, bitrate_idx=14, mode=0, mode_ext=-1, short_pct=20, mixed_pct=20, crc_pct=0)
    n, F = 40, 4
    buf, offs, sizes = _gen.batch(cfg, 505, n, F)

    def staging():
        return _decode(buf, offs, sizes, n, F), mp3_amd.BatchDecoder(n, F).huffman_only(buf, offs, sizes, F)
    _both(staging)


@pytest.mark.parametrize("path", ["wave", "lane"])
def test_demux_paths(path):
    """k_demux (one wave per stream) and k_walk + k_mdcopy (one lane per
    stream), forced by MP3D_DEMUX, on both families."""
    buf, offs, sizes = _mixed_family()

    def demux():
        return _decode(buf, offs, sizes, 48, 6, env={"MP3D_DEMUX": path})
    _both(demux)


def test_two_calls_vs_one():
    """Each stream's bytes in one call, and cut in the middle (frames cut
    short, reservoir and synthesis state carried) over two calls."""
    n, F = 37, 5
    buf, offs, sizes = _gen.batch(_gen.C5, 501, n, F)
    half = sizes // 2

    def two_calls():
        dec = mp3_amd.BatchDecoder(n, F)
        out = []
        for of, sz in ((offs, half), (offs + half, sizes - half)):
            pcm, infos = dec.decode(buf, of, sz, F)
            out.append((pcm.copy(), infos.copy(), dec.get_state(0, n)))
        return out

    def one_call():
        return _decode(buf, offs, sizes, n, F)
    _both(two_calls)
    _both(one_call)


@pytest.mark.parametrize("ra", [0, 16])
@pytest.mark.parametrize("name", ["keypress_128k_js", "lsf_scale_24k_is", "bench_c5_g1"])
def test_per_frame_api(name, ra):
    """k_frame (ra = 0) and the read-ahead's k_demux_fp runs (ra = 16), int16
    and float32 calls, the state at the end."""
    data, _ = _golden.case(name)
    script = [("call", False)] * 20 + [("state",)] + [("call", True)] * 20 + [("state",)]

    def per_frame():
        return RA._run(RA._dec(ra), data, script)
    out = _both(per_frame)
    assert sum(1 for r in out if r[0] != "state") >= 10


def test_huffman_only_and_synth_only():
    """A 16 x 4 batch: the integer stage alone (one wave per unit where the
    host selects it at this size) and the synth-only entry (k_synth<true>)."""
    n, F = 16, 4
    buf, offs, sizes = _gen.batch(_gen.C3, 7, n, F)
    xr, bt, mx = _gen.c2_spectra(n, F, 2, seed=31)

    def stages():
        is_out, sf_out = mp3_amd.BatchDecoder(n, F).huffman_only(buf, offs, sizes, F)
        dec = mp3_amd.BatchDecoder(n, F)
        return is_out, sf_out, dec.synth_only(xr, bt, mx, 2, 44100), dec.get_state(0, n)
    is_out, _, pcm, _ = _both(stages)
    assert is_out.any() and pcm.any()


def test_decode_long():
    """512 frames in 4-frame segments (k_gather_frames)."""
    data, _ = _golden.case("long_c3_512")

    def long_stream():
        pcm, infos, si = mp3_amd.BatchDecoder(64, 4 + 11).decode_long(data, 4)
        return pcm, infos, bytes(si)
    pcm, infos, _ = _both(long_stream)
    assert len(pcm) == 512 and (infos["samples"] == 1152).all()


@pytest.fixture(scope="module")
def packed_batch():
    return PK.Batch()


@pytest.mark.parametrize("f32", [True, False])
def test_decode_packed(packed_batch, f32):
    """The packed sink at (48000, 2): whole with a flush, and in calls of 5
    and 11 frames (k_rs_plan, k_rs_filter, k_rs_update)."""
    batch, fmt = packed_batch, (48000, 2)

    def packed():
        out, counts, infos = PK.run_whole(batch, fmt, f32=f32)
        chunks, per_call = PK.run_chunks(batch, fmt, [5, 11], f32=f32)
        return out, counts, infos, chunks, per_call
    _, counts, _, _, _ = _both(packed)
    assert counts.max() > 0
