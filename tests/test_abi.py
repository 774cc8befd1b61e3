"""The C-ABI library loads and exports every symbol include/mp3d.h declares
(no compute calls: this runs on CPU-only machines too)."""
import ctypes
import re

import mp3_amd
from mp3_amd import _build

HDR = _build.ROOT / "include" / "mp3d.h"


def declared():
    src = HDR.read_text()
    return sorted(set(re.findall(r"MP3D_API\s+[\w\s\*]*?\b(mp3d_\w+)\s*\(", src)))


def test_header_declares_api():
    names = declared()
    assert "mp3d_decode_frame" in names and "mp3d_batch_decode" in names
    assert len(names) == len(mp3_amd.EXPORTS)
    assert sorted(mp3_amd.EXPORTS) == names


SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
RETURNS = dict(SCALARS, **{"void": None, "const char *": ctypes.c_char_p})


def prototypes():
    """name -> (return type, [parameter declarations]) of every MP3D_API
    prototype, from the name's ( to the closing );"""
    src = re.sub(r"/\*.*?\*/", " ", HDR.read_text(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"MP3D_API\s+([\w\s\*]*?)\b(mp3d_\w+)\s*\(([^;]*?)\)\s*;", src):
        params = [" ".join(p.split()) for p in params.split(",")]
        protos[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return protos


def test_prototypes_parse():
    protos = prototypes()
    assert sorted(protos) == declared()
    assert protos["mp3d_state_bytes"] == ("size_t", [])
    assert protos["mp3d_strerror"] == ("const char *", ["int err"])
    assert protos["mp3d_decode_frame"][1][2:4] == ["size_t bytes", "int16_t *pcm"]  # (a comment inside is dropped)
    assert len(protos["mp3d_batch_limit"][1]) == 13 and len(protos["mp3d_batch_decode_limited"][1]) == 15


def test_signature_table_matches_the_header():
    """Argument count, scalar widths and return type of every export, in the
    table and as bound on the loaded library."""
    protos, L = prototypes(), mp3_amd.lib()
    assert list(mp3_amd.ABI) == mp3_amd.EXPORTS
    for name in mp3_amd.EXPORTS:
        ret, params = protos[name]
        restype, argtypes = mp3_amd.ABI[name]
        assert restype is RETURNS[ret], name
        assert len(argtypes) == len(params), name
        for t, p in zip(argtypes, params):
            if "*" in p:
                assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer), (name, p)
            else:
                words = [w for w in p.split() if w != "const"]
                assert t is SCALARS[" ".join(words[:-1])], (name, p)  # (the last word is the parameter's name)
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_library_exports_all_declared_symbols():
    _build.build_hip()
    L = ctypes.CDLL(str(mp3_amd.LIB_PATH))
    for n in declared():
        assert hasattr(L, n), n
    assert L.mp3d_abi_version() == 5
    assert mp3_amd.state_bytes() > 8000  # the opaque per-stream state blob


def test_no_device_fails_loudly_or_creates():
    """Without a GPU, creation must fail with MP3D_E_NO_DEVICE (no CPU fallback)."""
    import torch
    L = mp3_amd.lib()
    h = ctypes.c_void_p()
    rc = L.mp3d_batch_create(0, 1, 1, ctypes.byref(h))
    if torch.cuda.device_count() == 0:
        assert rc == -2
    else:
        assert rc == 0
        L.mp3d_batch_destroy(h)
