"""CPU tests of the band selection and tile ranking in one launch (include/sdfr.h: sdfr_band_select_rank, sdfr_mlp_forward_balanced_deferred;
csrc/band_rank.hip): the argument checks, and header, exports and binding in step.  The launches themselves: tests/test_gpu_band_rank.py."""
import ctypes
import os
import re

from sdflabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.03


def test_argument_checks_need_no_device():
    """no decoder is dereferenced and no HIP call is made before the checks; exports, header and binding name the same two entry points"""
    L = _lib.lib()
    fake = ctypes.create_string_buffer(64)
    p = ctypes.addressof(fake)
    sel = [((None, 8, 1, THR, None, None, p, 4, p, None, None, 0, None, 0, None), b"NULL"),
           ((p, 8, 1, THR, None, None, None, 4, p, None, None, 0, None, 0, None), b"NULL"),
           ((p, 8, 1, THR, None, None, p, 4, None, None, None, 0, None, 0, None), b"NULL"),
           ((p, -1, 1, THR, None, None, p, 4, p, None, None, 0, None, 0, None), b"negative"),
           ((p, 8, -1, THR, None, None, p, 4, p, None, None, 0, None, 0, None), b"negative"),
           ((p, 8, 1, THR, None, None, p, -4, p, None, None, 0, None, 0, None), b"negative"),
           ((p, 8, 1, THR, None, None, p, 4, p, None, None, 0, p, 0, None), b"order_rows=0"),
           ((p, 8, 1, THR, None, None, p, 4, p, None, None, 0, p, -64, None), b"order_rows=-64"),
           ((p, 8, 1, THR, None, None, p, 4, p, None, None, 0, p, 2 ** 31, None), b"out of range")]
    for args, msg in sel:
        assert L.sdfr_band_select_rank(*args) == -1, args
        assert msg in L.sdfr_last_error() and b"sdfr_band_select_rank" in L.sdfr_last_error(), (msg, L.sdfr_last_error())
    fwd = [((None, p, 64, p, None, p, 64, None), b"NULL"), ((p, None, 64, p, None, p, 64, None), b"NULL"),
           ((p, p, 64, None, None, p, 64, None), b"NULL"), ((p, p, 64, p, None, None, 64, None), b"NULL"),
           ((p, p, 64, p, None, p, 0, None), b"order_rows=0"), ((p, p, 100, p, None, p, 64, None), b"not a multiple"),
           ((p, p, -64, p, None, p, 64, None), b"out of range")]
    for args, msg in fwd:
        assert L.sdfr_mlp_forward_balanced_deferred(*args) == -1, args
        assert msg in L.sdfr_last_error() and b"sdfr_mlp_forward_balanced_deferred" in L.sdfr_last_error(), (msg, L.sdfr_last_error())
    assert L.sdfr_band_select_rank_max_rows() >= 64000


def test_header_binding_and_version_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 422
    L = _lib.lib()
    assert L.sdfr_version() == _lib.ABI_VERSION
    for name in ("sdfr_band_select_rank", "sdfr_band_select_rank_max_rows", "sdfr_mlp_forward_balanced_deferred"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header) and getattr(L, name)
    # the header's argument list of the selection: sdfr_band_select_ex's without scratch, then the state and its order_rows
    ex = re.search(r"int sdfr_band_select_ex\(([^;]*)\);", header).group(1)
    rank = re.search(r"int sdfr_band_select_rank\(([^;]*)\);", header).group(1)
    norm = lambda t: [" ".join(a.split()) for a in t.split(",")]
    assert norm(rank) == [a for a in norm(ex) if a != "int32_t* scratch"][:-1] + ["void* balance_state", "int64_t order_rows", "void* stream"]
