"""Stage a variant's source tree and build it: every file the library is built
from (_build.HIP_SRCS + HIP_HDRS) copied as it is, except those the calling
script rewrites."""
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mp3_amd import _build  # noqa: E402

HOST = "mp3d_batch.cpp"  # the host source a debug export is appended to


def build(d, out, rewritten, extra=()):
    """rewritten: {file name: its new text}; d: the staging directory."""
    os.makedirs(d, exist_ok=True)
    assert set(rewritten) <= set(_build.HIP_SRCS + _build.HIP_HDRS), sorted(rewritten)
    for n in _build.HIP_SRCS + _build.HIP_HDRS:
        if n in rewritten:
            open(os.path.join(d, n), "w").write(rewritten[n])
        else:
            shutil.copy(os.path.join("mp3_amd/csrc", n), d)
    os.makedirs(d + "/../../include", exist_ok=True)  # (the sources include ../../include/mp3d.h)
    shutil.copy("include/mp3d.h", d + "/../../include/")
    _build.compile_hip(d, out, d + "/obj", extra=extra)
    print(out)
