"""The segment sink's kernels run MP3D_LDS_ENTRY() before anything else (no GPU
needed): the rule of tests/test_wglds_coverage.py, whose own source list is
fixed, applied to mp3d_segment.hip."""
import test_wglds_coverage as cov
from mp3_amd import _build

EXPECTED = {"k_sg_plan", "k_sg_energy", "k_sg_emit"}


def test_segment_kernels_poison_their_lds_at_entry():
    src = (_build.CSRC / "mp3d_segment.hip").read_text()
    found = cov.kernels(src)
    assert set(found) == EXPECTED
    for name, stmts in found.items():
        cov.check(name, stmts)
    # (the parser sees the declarations of k_sg_energy and k_sg_emit)
    assert sum("__shared__" in s for st in found.values() for s in st) == 2
    # static LDS only, no inline assembly
    body = cov.strip_comments(src)
    assert "extern __shared__" not in body and "asm" not in body
    # the quantisation is the packed sink's, through one function
    assert "pcm_i16(" in body and "pcm_i16(" in cov.strip_comments((_build.CSRC / "mp3d_resample.hip").read_text())


def test_the_files_are_built_into_both_libraries():
    assert "mp3d_segment.hip" in _build.HIP_SRCS and "mp3d_segment.cpp" in _build.HIP_SRCS
    assert "mp3d_segment.h" in _build.HIP_HDRS
