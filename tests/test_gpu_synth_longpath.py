"""k_synth's all-long path: M/S granules with long
blocks in both channels take a straight-line phase Q per class of live
128-line chunks (2, 3, 4 or 5 by the granule's largest nz_end) and the alias
step in place under EXEC masks.  MP3D_SYNTH_LONGPATH=0 launches the kernel
whose every granule takes the general forms; the two must agree bit for bit
(PCM of both sinks, frame infos, state blobs), on batches where the path
flips granule by granule, on every chunk class and class boundary, on
escapes (|is| >= 256), and with the state carried from call to call.

The generator settings were chosen on the CPU from the generator's truth
(is[] per granule): the batches below hold a silent granule, granules of
every class, and granules whose last nonzero line is exactly 255, 256, 383,
384, 511 and 512 -- all of them long / long M/S, so they run the new path."""
import numpy as np
import pytest

import _gen
import mp3_amd
from _state import state_view
from test_gpu_parity import oracle_pcm16, split_frames

pytestmark = pytest.mark.gpu

F = 8
N = 16  # streams per generator setting


def _concat(parts):
    buf = np.concatenate([p[0] for p in parts])
    offs, sizes, base = [], [], 0
    for b, o, s in parts:
        offs.append(o + base)
        sizes.append(s)
        base += len(b)
    return buf, np.concatenate(offs).astype(np.uint64), np.concatenate(sizes).astype(np.uint32)


def _decode_all(batch, monkeypatch, longpath):
    """PCM of both sinks, infos and the state blobs from fresh decoders"""
    buf, offs, sizes = batch
    n = len(offs)
    if longpath:
        monkeypatch.delenv("MP3D_SYNTH_LONGPATH", raising=False)
    else:
        monkeypatch.setenv("MP3D_SYNTH_LONGPATH", "0")
    out = {}
    for f32 in (False, True):
        dec = mp3_amd.BatchDecoder(n, F)
        pcm, infos = dec.decode(buf, offs, sizes, F, f32=f32)
        out["pcm%d" % f32] = np.array(pcm, copy=True)
        out["inf%d" % f32] = np.array(infos, copy=True)
        out["st%d" % f32] = np.array(dec.get_state(0, n), copy=True)
    monkeypatch.delenv("MP3D_SYNTH_LONGPATH", raising=False)
    return out


def _same(a, b):
    for k in sorted(a):
        # (bytes: NaN-proof and exact for the float sink and the state blobs)
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _tap(batch):
    """is[] rows by the Huffman tap [n, F, gr, ch, 576] and each granule's
    largest last nonzero line over its channels (-1: silent)"""
    buf, offs, sizes = batch
    n = len(offs)
    is_rows, _ = mp3_amd.BatchDecoder(n, F).huffman_only(buf, offs, sizes, F)
    rows = np.asarray(is_rows).reshape(n, F, 2, 2, 576)
    nz = rows != 0
    last = np.where(nz.any(-1), 575 - np.argmax(nz[..., ::-1], axis=-1), -1)
    return rows, last.max(axis=-1)


def _vs_oracle(batch, pcm, infos, streams):
    buf, offs, sizes = batch
    for s in streams:
        o = oracle_pcm16(bytes(buf[offs[s]:offs[s] + sizes[s]]))
        got = mp3_amd.pcm_to_planar(pcm[s], infos[s])
        assert got.shape == o.shape, s
        assert np.abs(got.astype(np.int32) - o.astype(np.int32)).max() <= 1, s


@pytest.fixture(scope="module")
def flip_batch():
    """the predicate flips granule by granule and stream by stream: M/S, L/R
    (the fused requantiser's), intensity (falls back), half the granules
    short or mixed in one channel or both, mono"""
    variants = [dict(mode_ext=2), dict(mode_ext=0), dict(mode_ext=1), dict(mode_ext=3),
                dict(short_pct=50, mixed_pct=50), dict(mode=3)]
    return _concat([_gen.batch(dict(_gen.C3, **v), 8_800_001 + 1009 * k, N, F) for k, v in enumerate(variants)])


# long blocks only (every stereo granule runs the new path), from nearly
# silent to a full bit budget; (fill_pct, bitrate_idx, seed_base)
CLASS_SETTINGS = [(3, 9, 9_300_001), (100, 14, 10_302_962), (100, 14, 9_602_941)]


@pytest.fixture(scope="module")
def class_batch():
    return _concat([_gen.batch(dict(_gen.C3, short_pct=0, mixed_pct=0, fill_pct=fill, bitrate_idx=br), seed, N, F)
                    for fill, br, seed in CLASS_SETTINGS])


@pytest.fixture(scope="module")
def class_tap(class_batch):
    return _tap(class_batch)


def test_paths_agree_where_the_predicate_flips(flip_batch, monkeypatch):
    off = _decode_all(flip_batch, monkeypatch, False)
    on = _decode_all(flip_batch, monkeypatch, True)
    _same(on, off)
    # the batch is not trivially silent, and the M/S streams are stereo
    assert np.abs(on["pcm0"][:N].astype(np.int32)).max() > 1000


def test_chunk_classes_and_boundaries(class_batch, class_tap, monkeypatch):
    _, gmax = class_tap
    assert (gmax < 0).any(), "no silent granule"
    assert ((gmax >= 0) & (gmax < 256)).any()
    assert ((gmax >= 256) & (gmax < 384)).any()
    assert ((gmax >= 384) & (gmax < 512)).any()
    assert (gmax >= 512).any()
    checked = set(range(0, len(gmax), 4))
    for v in (255, 256, 383, 384, 511, 512):
        where = np.argwhere(gmax == v)
        assert len(where), "no granule whose last nonzero line is %d" % v
        checked.add(int(where[0][0]))
    on = _decode_all(class_batch, monkeypatch, True)
    off = _decode_all(class_batch, monkeypatch, False)
    _same(on, off)
    _vs_oracle(class_batch, on["pcm0"], on["inf0"], sorted(checked))


def test_escapes_on_the_long_path(class_batch, class_tap, monkeypatch):
    rows, _ = class_tap
    # long blocks only and M/S (C3): every granule with an escape runs the new path's patch block
    big = (np.abs(rows.astype(np.int32)) >= 256).any(axis=(-1, -2))  # [n, F, gr]
    streams = [int(s) for s in np.argwhere(big.any(axis=(1, 2)))[:, 0]]
    assert len(streams) >= 8 and int(big.sum()) >= 20, (len(streams), int(big.sum()))
    on = _decode_all(class_batch, monkeypatch, True)
    off = _decode_all(class_batch, monkeypatch, False)
    _same(on, off)
    _vs_oracle(class_batch, on["pcm0"], on["inf0"], streams[:8])


def test_state_carried_across_calls(flip_batch):
    """two calls of 4 frames = one call of 8, with the path on"""
    buf, offs, sizes = flip_batch
    n = len(offs)

    def chunk(k0, k1):
        parts = []
        for s in range(n):
            data = bytes(buf[offs[s]:offs[s] + sizes[s]])
            fo = split_frames(data) + [len(data)]
            parts.append(data[fo[k0]:fo[k1]])
        sz = np.array([len(p) for p in parts], np.uint32)
        of = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
        return np.frombuffer(b"".join(parts), np.uint8), of, sz

    for f32 in (False, True):
        one = mp3_amd.BatchDecoder(n, F)
        ref, rinf = one.decode(buf, offs, sizes, F, f32=f32)
        ref, rinf, rst = np.array(ref, copy=True), np.array(rinf, copy=True), np.array(one.get_state(0, n), copy=True)
        two = mp3_amd.BatchDecoder(n, F)
        p1, i1 = two.decode(*chunk(0, 4), 4, f32=f32)
        p1, i1 = np.array(p1, copy=True), np.array(i1, copy=True)
        p2, i2 = two.decode(*chunk(4, 8), 4, f32=f32)
        assert np.concatenate([p1, p2], axis=1).tobytes() == ref.tobytes()
        assert np.concatenate([i1, i2], axis=1).tobytes() == rinf.tobytes()
        # the blobs' meaningful part: the reservoir bytes past res_len are stale
        # and differ with the calls' lengths (tests/_state.py)
        assert state_view(two.get_state(0, n)).tobytes() == state_view(rst).tobytes()
