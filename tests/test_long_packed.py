"""The host side of BatchDecoder.decode_long_packed (no GPU needed): the new
exports, mp3d_long_packed_bound against a plain formula, and info_frame(), the
builder of tagged streams that tests/test_gpu_long_packed.py trims, checked
against the oracle's reading of the tag and the library's frame walk."""
import math

import numpy as np
import pytest

import _gen
import _golden
import _oracle
import mp3_amd

BITRATE_V1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
BITRATE_LSF = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]
HZ_V1 = [44100, 48000, 32000]


def header_fields(h):
    """(lsf, hz, mono) of a Layer III header."""
    ver = (h[1] >> 3) & 3  # 3 MPEG-1, 2 MPEG-2, 0 MPEG-2.5
    hz = HZ_V1[(h[2] >> 2) & 3] // (1 if ver == 3 else 2 if ver == 2 else 4)
    return ver != 3, hz, (h[3] >> 6) == 3


def info_frame(first_header4, frames, delay, padding, with_count=True):
    """One valid Layer III frame at the stream's own version, rate and channel
    mode holding an Info tag with a LAME extension, in the layout
    parse_info_tag (mp3d_demux_dev.h) and FFmpeg's demuxer read: no CRC, the
    smallest bitrate whose frame holds the tag, zero side info, "Info", BE32
    flags (1 with a frame count, else 0), the frame count, a 9-byte
    "LAME3.100" string and, 21 bytes from its start, BE24 delay << 12 |
    padding."""
    h = bytes(first_header4)
    lsf, hz, mono = header_fields(h)
    side = (9 if mono else 17) if lsf else (17 if mono else 32)
    tag = b"Info" + (1 if with_count else 0).to_bytes(4, "big") + (int(frames).to_bytes(4, "big") if with_count else b"")
    tag += b"LAME3.100".ljust(21, b"\0") + ((int(delay) << 12) | int(padding)).to_bytes(3, "big")
    need = 4 + side + len(tag)
    for bi in range(1, 15):
        fb = (72000 * BITRATE_LSF[bi] if lsf else 144000 * BITRATE_V1[bi]) // hz
        if fb >= need:
            break
    else:
        raise ValueError("no bitrate holds the tag")
    head = bytes([h[0], h[1] | 1, (bi << 4) | (h[2] & 0x0C), h[3]])  # no CRC, no padding byte
    return (head + b"\0" * side + tag).ljust(fb, b"\0")


def tagged(stream, frames, delay, padding, with_count=True):
    return info_frame(stream[:4], frames, delay, padding, with_count) + stream


def audio_stream(name):
    """A golden's bytes from its first frame header on."""
    data, _ = _golden.case(name)
    return data[int(mp3_amd.long_plan(data)[0][0]):]


@pytest.mark.parametrize("name,spf", [("c3_s0", 1152), ("c5_mono_48k_crc", 1152), ("lsf_22k_js", 576)])
@pytest.mark.parametrize("with_count", [True, False])
def test_info_frame_reads_back(name, spf, with_count):
    """MPEG-1 stereo, MPEG-1 mono and LSF stereo: the oracle reads what was
    put in, and the frame walk sees the tag frame as slot 0."""
    stream = audio_stream(name)
    data = tagged(stream, 40, 1700, 2000, with_count)
    found, tag = _oracle.info_tag(data)
    assert found
    want = dict(has_lame=1, enc_delay=1700, enc_padding=2000, total_frames=40 if with_count else -1,
                skip_samples=1700 + 529, end_sample=40 * spf + 529 - 2000 if with_count else -1)
    for k, v in want.items():
        assert tag[k] == v, (k, tag[k], v)
    own = mp3_amd.long_plan(stream)[0]
    off = mp3_amd.long_plan(data)[0]
    assert off[0] == 0 and np.array_equal(off[1:], own + (len(data) - len(stream)))


def test_generated_stream_takes_a_tag():
    stream, _ = _gen.stream(_gen.C3, 7, 40)
    data = tagged(stream, 40, 576, 1500)
    found, tag = _oracle.info_tag(data)
    assert found and tag["has_lame"] == 1 and tag["skip_samples"] == 576 + 529
    assert tag["end_sample"] == 40 * 1152 + 529 - 1500
    assert len(mp3_amd.long_plan(data)[0]) == 41


@pytest.mark.parametrize("name", ["keypress_128k_js", "lsf_8k_js", "c5_mono_48k_crc"])
@pytest.mark.parametrize("out_hz", [48000, 44100, 8000])
def test_bound_is_the_formula(name, out_hz):
    data, _ = _golden.case(name)
    off = mp3_amd.long_plan(data)[0]
    lsf, hz, _ = header_fields(data[int(off[0]):int(off[0]) + 4])
    g = math.gcd(hz, out_hz)
    L, M = out_hz // g, hz // g
    want = -(-len(off) * (576 if lsf else 1152) * L // M)
    assert mp3_amd.long_packed_bound(data, out_hz) == want
    assert mp3_amd.long_packed_bound(np.frombuffer(data, np.uint8), out_hz) == want


def test_bound_refuses_a_bad_rate():
    data, _ = _golden.case("keypress_128k_js")
    with pytest.raises(mp3_amd.MP3DError, match="-1"):
        mp3_amd.long_packed_bound(data, 44000)
    assert mp3_amd.long_packed_bound(b"no frames here", 48000) == 0


def test_exports():
    names = sorted(mp3_amd.EXPORTS)
    assert "mp3d_batch_decode_long_packed" in names and "mp3d_long_packed_bound" in names
    L = mp3_amd.lib()
    assert hasattr(L, "mp3d_batch_decode_long_packed") and hasattr(L, "mp3d_long_packed_bound")
    assert mp3_amd.LONG_GAPLESS == 1
