"""The equaliser sink's kernels run MP3D_LDS_ENTRY() before anything else (no GPU
needed): the rule of tests/test_wglds_coverage.py, whose own source list is
fixed, applied to mp3d_eq.hip."""
import test_wglds_coverage as cov
from mp3_amd import _build

EXPECTED = {"k_eq_plan", "k_eq_local", "k_eq_carry", "k_eq_apply"}


def test_eq_kernels_poison_their_lds_at_entry():
    src = (_build.CSRC / "mp3d_eq.hip").read_text()
    found = cov.kernels(src)
    assert set(found) == EXPECTED
    for name, stmts in found.items():
        cov.check(name, stmts)
    # (the parser sees the declarations: two each in k_eq_local, k_eq_carry and k_eq_apply)
    assert sum("__shared__" in s for st in found.values() for s in st) == 6
    # static LDS only, no inline assembly
    body = cov.strip_comments(src)
    assert "extern __shared__" not in body and "asm" not in body
    # the two builds round alike: no implicit contraction
    assert "#pragma clang fp contract(off)" in body


def test_the_files_are_built_into_both_libraries():
    assert "mp3d_eq.hip" in _build.HIP_SRCS and "mp3d_eq.cpp" in _build.HIP_SRCS
    assert "mp3d_eq.h" in _build.HIP_HDRS
