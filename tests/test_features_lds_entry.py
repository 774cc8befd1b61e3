"""The feature sink's kernels run MP3D_LDS_ENTRY() before anything else (no
GPU needed): the rule of tests/test_wglds_coverage.py, whose own source list
is fixed, applied to mp3d_features.hip."""
import test_wglds_coverage as cov
from mp3_amd import _build

EXPECTED = {"k_ft_plan", "k_ft_transform", "k_ft_update"}


def test_feature_kernels_poison_their_lds_at_entry():
    found = cov.kernels((_build.CSRC / "mp3d_features.hip").read_text())
    assert set(found) == EXPECTED
    for name, stmts in found.items():
        cov.check(name, stmts)
    assert sum("__shared__" in s for st in found.values() for s in st) >= 7  # (the parser sees the declarations)


def test_the_file_is_built_into_both_libraries():
    assert "mp3d_features.hip" in _build.HIP_SRCS and "mp3d_features.h" in _build.HIP_HDRS
