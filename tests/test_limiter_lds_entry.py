"""The limiter's kernels run MP3D_LDS_ENTRY() before anything else (no GPU
needed): the rule of tests/test_wglds_coverage.py, whose own source list is
fixed, applied to mp3d_limiter.hip."""
import test_wglds_coverage as cov
from mp3_amd import _build

EXPECTED = {"k_lim_plan", "k_lim_tile", "k_lim_carry"}


def test_limiter_kernels_poison_their_lds_at_entry():
    src = (_build.CSRC / "mp3d_limiter.hip").read_text()
    found = cov.kernels(src)
    assert set(found) == EXPECTED
    for name, stmts in found.items():
        cov.check(name, stmts)
    # (the parser sees the declarations of k_lim_tile and k_lim_carry)
    assert sum("__shared__" in s for st in found.values() for s in st) == 7
    # static LDS only, no inline assembly
    body = cov.strip_comments(src)
    assert "extern __shared__" not in body and "asm" not in body
    # the detector's chain is the true-peak tap's, through one header
    assert '#include "mp3d_tp_chain.h"' in body
    assert '#include "mp3d_tp_chain.h"' in cov.strip_comments((_build.CSRC / "mp3d_normalize.hip").read_text())
    assert "fmaf" not in body and "elementwise_fma" not in body


def test_the_files_are_built_into_both_libraries():
    assert "mp3d_limiter.hip" in _build.HIP_SRCS and "mp3d_limiter.cpp" in _build.HIP_SRCS
    assert "mp3d_limiter.h" in _build.HIP_HDRS and "mp3d_tp_chain.h" in _build.HIP_HDRS
