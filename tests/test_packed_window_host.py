"""No GPU: the public surface of the per-stream sample windows of the packed
and the feature sink (mp3d_batch_set_window / mp3d_batch_sink_window,
MP3D_PACK_GAPLESS; include/mp3d.h "Sample windows")."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import mp3_amd

HEADER = pathlib.Path(__file__).resolve().parent.parent / "include" / "mp3d.h"
NEW = ["mp3d_batch_set_window", "mp3d_batch_sink_window"]


def test_constants():
    assert mp3_amd.PACK_GAPLESS == 2 and mp3_amd.PACK_FLUSH == 1
    assert mp3_amd.WINDOW_NO_END == 2 ** 63 - 1 == ctypes.c_longlong(-1).value + 2 ** 63
    src = HEADER.read_text()
    assert re.search(r"#define\s+MP3D_PACK_GAPLESS\s+2\b", src)
    assert re.search(r"#define\s+MP3D_WINDOW_NO_END\s+LLONG_MAX\b", src)
    assert re.search(r"#define\s+MP3D_ABI_VERSION\s+5\b", src)  # additive: the version stays


def test_exports():
    L = mp3_amd.lib()
    for name in NEW:
        assert name in mp3_amd.EXPORTS
        assert hasattr(L, name), name
    assert L.mp3d_abi_version() == 5


class Refuses:
    """Stands in for the library: any call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached the library (%s)" % name)


def wrapper():
    dec = mp3_amd.BatchDecoder.__new__(mp3_amd.BatchDecoder)
    dec._L, dec._h, dec.max_streams = Refuses(), None, 4
    return dec


@pytest.mark.parametrize("lo,hi", [([0, -1], None), ([-5], [7]), ([3], [2]), ([0, 10], [5, 9]), ([0, 1], [5])])
def test_wrapper_refuses_bad_windows_before_any_call(lo, hi):
    with pytest.raises(ValueError):
        wrapper().set_window(lo, hi)


def test_wrapper_refuses_hi_without_lo():
    with pytest.raises(ValueError):
        wrapper().set_window(None, [5])


def test_null_handle_is_an_argument_error():
    """The library's own -1 (no handle: nothing touches a GPU)."""
    L = mp3_amd.lib()
    lo = np.zeros(1, np.int64)
    assert L.mp3d_batch_set_window(None, 0, 1, lo.ctypes.data, None) == -1
    assert L.mp3d_batch_sink_window(None, 0, 1, lo.ctypes.data, None, None) == -1
