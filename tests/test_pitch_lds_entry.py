"""The pitch sink's kernels run MP3D_LDS_ENTRY() before anything else (no GPU
needed): the rule of tests/test_wglds_coverage.py, whose own source list is
fixed, applied to mp3d_pitch.hip."""
import test_wglds_coverage as cov
from mp3_amd import _build

EXPECTED = {"k_pt_plan", "k_pt_frames", "k_pt_update"}


def test_pitch_kernels_poison_their_lds_at_entry():
    src = (_build.CSRC / "mp3d_pitch.hip").read_text()
    found = cov.kernels(src)
    assert set(found) == EXPECTED
    for name, stmts in found.items():
        cov.check(name, stmts)
    # (the parser sees the declarations of k_pt_frames and k_pt_update)
    assert sum("__shared__" in s for s in found["k_pt_frames"]) >= 1
    assert sum("__shared__" in s for s in found["k_pt_update"]) == 1
    assert not any("__shared__" in s for s in found["k_pt_plan"])
    # static LDS only, no inline assembly
    body = cov.strip_comments(src)
    assert "extern __shared__" not in body and "asm" not in body
    # the quantisation is the packed sink's, through one function, and the dot product is the tempo sink's
    assert "pcm_i16(" in body and "pcm_i16(" in cov.strip_comments((_build.CSRC / "mp3d_resample.hip").read_text())
    assert "__builtin_amdgcn_sdot2(" in body


def test_the_files_are_built_into_both_libraries():
    assert "mp3d_pitch.hip" in _build.HIP_SRCS and "mp3d_pitch.cpp" in _build.HIP_SRCS
    assert "mp3d_pitch.h" in _build.HIP_HDRS
