"""The tempo sink's kernels run MP3D_LDS_ENTRY() before anything else (no GPU
needed): the rule of tests/test_wglds_coverage.py, whose own source list is
fixed, applied to mp3d_stretch.hip."""
import test_wglds_coverage as cov
from mp3_amd import _build

EXPECTED = {"k_st_plan", "k_st_blocks"}


def test_stretch_kernels_poison_their_lds_at_entry():
    src = (_build.CSRC / "mp3d_stretch.hip").read_text()
    found = cov.kernels(src)
    assert set(found) == EXPECTED
    for name, stmts in found.items():
        cov.check(name, stmts)
    assert sum("__shared__" in s for st in found.values() for s in st) == 5  # (the parser sees k_st_blocks' declarations)
    # static LDS only, no inline assembly
    body = cov.strip_comments(src)
    assert "extern __shared__" not in body and "asm" not in body


def test_the_files_are_built_into_both_libraries():
    assert "mp3d_stretch.hip" in _build.HIP_SRCS and "mp3d_stretch.cpp" in _build.HIP_SRCS
    assert "mp3d_stretch.h" in _build.HIP_HDRS
