"""k_huffman's burst stores and wave count (the lane kernel: one lane per unit).

A lane keeps the first groups of each 128-B line of its is[] row in registers
and stores the line's 8 groups back to back; the last, partial burst is
flushed before the count1 stores overwrite its tail.  What can go wrong is
where a burst is partial: rows shorter than one line, rows that end on a line
boundary, just after one and just before one, long rows, and rounds whose
lanes run far past a short lane's own big_values (that lane then holds and
flushes zero groups over lines it has already written).  The coverage test
asserts, from the oracle's side info, that the two batches hold all of these.

The C ABI returns is[] rows and scalefactors, not UnitMeta.nz_end.  Every
row is compared whole with the oracle's tap (whose buffer starts zeroed, as
the batch call's does): equal below nz_end, zero at and past it, whatever
nz_end is.  The stored nz_end itself is what k_synth masks each row with, so
it is checked through PCM, on rows that hold a longer unit's lines past it
(test_reused_rows_pcm): one too large lets stale lines in, one too small
drops lines."""
import os

import numpy as np
import pytest

import _gen
import _golden
import _oracle
import mp3_amd

pytestmark = pytest.mark.gpu

N, F = 48, 8  # 1 536 units: past the 1 024 up to which a batch takes the one-wave-per-unit kernel
SEEDS = {"c3": (_gen.C3, 7001), "c5": (_gen.C5, 7002)}  # (chosen on the CPU: test_coverage holds for them)
_cache = {}


def oracle_units(cfg, seed, n, nf):
    """is[] rows [n, nf, 2, 2, 576] and side-info taps [n, nf, 2, 2, 20] of the
    per-frame oracle; coded[n, nf, 2, 2]: the unit exists (granule and channel)"""
    is_ref = np.zeros((n, nf, 2, 2, 576), np.int16)
    side = np.zeros((n, nf, 2, 2, 20), np.int32)
    coded = np.zeros((n, nf, 2, 2), bool)
    for s in range(n):
        data, offs = _gen.stream(cfg, seed + s, nf)
        ends = list(offs[1:]) + [len(data)]
        dec = _oracle.Decoder()
        for f in range(nf):
            r, _, info = dec.decode_frame(data[offs[f]:ends[f]])
            assert r > 0, (s, f, r)
            i, _, _, sd = dec.taps()
            ngr = r // 576
            is_ref[s, f, :ngr, :info.channels] = i[:ngr, :info.channels]
            side[s, f] = sd
            coded[s, f, :ngr, :info.channels] = True
    return is_ref, side, coded


def batch(name):
    """the named batch, its oracle rows and side info: computed once"""
    if name not in _cache:
        cfg, seed = SEEDS[name]
        _cache[name] = (_gen.batch(cfg, seed, N, F), oracle_units(cfg, seed, N, F))
    return _cache[name]


def huffman_only(path, buf, offs, sizes, n, nf):
    os.environ["MP3D_HUFF"] = path
    try:
        return mp3_amd.BatchDecoder(n, nf).huffman_only(buf, offs, sizes, nf)
    finally:
        os.environ.pop("MP3D_HUFF", None)


def coverage(bv2):
    """bv2: 2 * big_values of the decoded units of one batch, in unit order"""
    # k_rank's rounds: 64 consecutive units of the descending big_values order
    # (the order inside a bin does not change a round's extremes)
    srt = np.sort(bv2)[::-1]
    spread = max(int(srt[i] - srt[min(i + 63, srt.size - 1)]) for i in range(0, srt.size, 64))
    return {"short": int((bv2 < 64).sum()), "mod0": int(((bv2 % 64 == 0) & (bv2 > 0)).sum()),
            "mod_lo": int(((bv2 % 64 > 0) & (bv2 % 64 < 16)).sum()), "mod_hi": int((bv2 % 64 >= 48).sum()),
            "long": int((bv2 >= 384).sum()), "round_spread": spread}


def test_coverage():
    """hard assertions on what the two batches exercise, from the oracle's side info"""
    tot = {}
    for name in SEEDS:
        (buf, offs, sizes), (is_ref, side, coded) = batch(name)
        c = coverage(2 * side[..., 1][coded])
        print(name, c)
        for k, v in c.items():
            tot[k] = max(tot.get(k, 0), v)
    assert tot["short"] >= 1, "a unit with 2 * big_values < 64 (no full burst)"
    assert tot["mod0"] >= 1, "a big_values region ending on a line boundary (nothing held at the flush)"
    assert tot["mod_lo"] >= 1, "a region ending in a line's first group"
    assert tot["mod_hi"] >= 1, "a region ending in a line's last group"
    assert tot["long"] >= 1, "a unit with 2 * big_values >= 384"
    assert tot["round_spread"] > 128, "a round whose lanes differ by more than 128 lines of big_values"


@pytest.mark.parametrize("name", list(SEEDS))
def test_rows_vs_oracle_and_wave_kernel(name):
    (buf, offs, sizes), (is_ref, side, coded) = batch(name)
    is_lane, sf_lane = huffman_only("lane", buf, offs, sizes, N, F)
    bad = np.argwhere((is_lane != is_ref).any(-1))
    assert bad.size == 0, (name, "units whose row differs from the oracle's", bad[:8].tolist())
    # the one-wave-per-unit kernel (not touched by the burst stores), bit for bit
    is_wave, sf_wave = huffman_only("wave", buf, offs, sizes, N, F)
    assert np.array_equal(is_lane, is_wave)
    assert np.array_equal(sf_lane, sf_wave)


def pcm_vs_oracle(pcm, infos, streams, skip=0):
    """worst |GPU - oracle| in LSB over the streams; the oracle decodes each
    whole stream, the GPU PCM is its part after `skip` samples"""
    worst = 0
    for s, data in enumerate(streams):
        o = _golden.to_int16(_oracle.decode_stream(data)[0])[:, skip:]
        got = mp3_amd.pcm_to_planar(pcm[s], infos[s])
        assert got.shape == o.shape, (s, got.shape, o.shape)
        worst = max(worst, int(np.abs(got.astype(np.int32) - o.astype(np.int32)).max()))
    return worst


def test_reused_rows_pcm():
    """Rows that held long units, then short ones: k_synth masks each row at
    nz_end, and nothing relies on zeros past the flushed burst.  One decoder
    decodes a full batch (320 kbit/s, every frame filled), then on the same
    streams a batch whose frames are 3 % filled; the oracle decodes each
    stream's two parts as one stream."""
    hi = dict(_gen.C3, bitrate_idx=14, fill_pct=100)
    lo = dict(hi, fill_pct=3)
    a, b = _gen.batch(hi, 7101, N, F), _gen.batch(lo, 7201, N, F)
    dec = mp3_amd.BatchDecoder(N, F)
    os.environ["MP3D_HUFF"] = "lane"
    try:
        dec.decode(*a, F)
        pcm, infos = dec.decode(*b, F)
    finally:
        os.environ.pop("MP3D_HUFF", None)
    streams = [bytes(a[0][a[1][s]:a[1][s] + a[2][s]]) + bytes(b[0][b[1][s]:b[1][s] + b[2][s]]) for s in range(N)]
    assert pcm_vs_oracle(pcm, infos, streams, skip=F * 1152) <= 1


def test_partial_last_round_pcm():
    """1 400 units: 21 full rounds and one of 56 lanes"""
    n, nf = 50, 7
    buf, offs, sizes = _gen.batch(_gen.C3, 7301, n, nf)
    os.environ["MP3D_HUFF"] = "lane"
    try:
        pcm, infos = mp3_amd.BatchDecoder(n, nf).decode(buf, offs, sizes, nf)
    finally:
        os.environ.pop("MP3D_HUFF", None)
    streams = [bytes(buf[offs[s]:offs[s] + sizes[s]]) for s in range(n)]
    assert pcm_vs_oracle(pcm, infos, streams) <= 1
