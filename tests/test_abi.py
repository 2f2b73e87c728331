"""CPU: the C-ABI library builds for gfx950, loads, and exports exactly what include/zsaac.h
declares (no compute calls — there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zsaac.h")


def _header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\bint\s+(zs_\w+)\s*\(", src))


@pytest.fixture(scope="module")
def libpath():
    from zsaac import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.LIB_PATH


def test_header_matches_binding_table():
    from zsaac._lib import SIGNATURES
    assert _header_symbols() == set(SIGNATURES)


def test_library_exports_every_header_symbol(libpath):
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT\s+(zs_\w+)", out))
    missing = _header_symbols() - exported
    assert not missing, missing
    assert exported <= _header_symbols(), exported - _header_symbols()


def test_code_object_targets_gfx950(libpath):
    # the .hip_fatbin section bundles one code object per offload target
    data = open(libpath, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    assert b"gfx942" not in data and b"gfx90a" not in data


def test_load_and_error_path(libpath):
    from zsaac import _lib
    lib = _lib.lib()
    assert lib.zs_version() == 1
    # argument validation runs on the host before any launch: a bad shape fails cleanly
    rc = lib.zs_gemm(4, 8, 30, 0, None, 32, None, 32, None, None, 0, None, 8, 0, 0, 1, None, None)
    assert rc == -1
    assert "multiple of 32" in _lib.last_error()
    with pytest.raises(_lib.ZsError):
        _lib.call("zs_tune_set", b"no_such_knob", 1)
    assert lib.zs_gemm_workspace_floats(64, 768, 3072) > 0
    # 4 row blocks of 64: a 256-row launch needs 4x the slabs of a 64-row one (same counters)
    w64, w256 = lib.zs_gemm_workspace_floats(64, 768, 3072), lib.zs_gemm_workspace_floats(256, 768, 3072)
    assert w256 - 4096 == 4 * (w64 - 4096)
    assert lib.zs_gemm_workspace_floats(257, 768, 3072) == 0
    assert lib.zs_lmhead_nblk(50257) == 393


def test_tune_set_decode_attn5_admits_only_live_values(libpath):
    """The decode_attn5 knob selects decode_attn6_kernel's phase length and reductions: 2, 3, 4
    and 6.  The values whose kernels are retired (0, 1, 5) and an unknown one (7) fail with
    ZS_ERR_ARG and a message naming the value; the knob is left at its default 6."""
    from zsaac import _lib
    lib = _lib.lib()
    try:
        for v in (0, 1, 5, 7):
            with pytest.raises(_lib.ZsError, match=rf"decode_attn5 = {v}\b"):
                _lib.call("zs_tune_set", b"decode_attn5", v)
            assert lib.zs_tune_set(b"decode_attn5", v) == -1          # ZS_ERR_ARG
        for v in (0, 1, 5):
            lib.zs_tune_set(b"decode_attn5", v)
            assert "retired" in _lib.last_error()
        for v in (2, 3, 4, 6):
            assert _lib.call("zs_tune_set", b"decode_attn5", v) == 0
    finally:
        _lib.call("zs_tune_set", b"decode_attn5", 6)


def test_tune_set_phase_launch_window_bounds(libpath):
    """dg_win_lo / dg_win_hi narrow the grid decode's phase launches to the launches [lo, hi) of a
    step's 62: lo in 0 .. 61, hi in 1 .. 62, anything else fails with ZS_ERR_ARG and a message
    naming the value, and leaves the knob where it was (0 / 62 at the end).  An empty window and
    a narrowed one with steps != 1 are refused by the phase entry points themselves, after their
    argument checks and before any launch (tests/test_gpu_grid_kernels.py, which has the device
    buffers those checks want)."""
    from zsaac import _lib, ops
    lib = _lib.lib()
    assert ops.DECODE_PHASE_LAUNCHES == 62
    try:
        for k, bad in ((b"dg_win_lo", (-1, 62, 1000)), (b"dg_win_hi", (0, -3, 63))):
            for v in bad:
                with pytest.raises(_lib.ZsError, match=rf"{k.decode()} = {v}\b"):
                    _lib.call("zs_tune_set", k, v)
                assert lib.zs_tune_set(k, v) == -1                    # ZS_ERR_ARG
        for lo, hi in ((0, 1), (61, 62), (17, 18), (60, 62), (0, 62)):
            assert _lib.call("zs_tune_set", b"dg_win_lo", lo) == 0
            assert _lib.call("zs_tune_set", b"dg_win_hi", hi) == 0
    finally:
        _lib.call("zs_tune_set", b"dg_win_lo", 0)
        _lib.call("zs_tune_set", b"dg_win_hi", 62)


def test_phase_window_wrapper_restores_the_default(libpath, monkeypatch):
    """ops.gpt2_decode_phase_window sets the window, runs one step's launches and restores 0 / 62
    in a finally -- also when the launch raises -- so a later call or captured graph never sees a
    narrowed window.  Out-of-range and empty windows are refused before any knob moves."""
    from zsaac import ops
    from zsaac._lib import ZsError
    seen = []
    monkeypatch.setattr(ops, "call", lambda name, *a: seen.append((name,) + a) or 0)

    def boom(*a, **kw):
        seen.append(("run", kw))
        raise ZsError("launch failed")
    monkeypatch.setattr(ops, "gpt2_decode_phases", boom)
    with pytest.raises(ZsError, match="launch failed"):
        ops.gpt2_decode_phase_window(first=7, last=8, grid=48)
    assert seen == [("zs_tune_set", b"dg_win_lo", 7), ("zs_tune_set", b"dg_win_hi", 8),
                    ("run", {"steps": 1, "grid": 48}),
                    ("zs_tune_set", b"dg_win_lo", 0), ("zs_tune_set", b"dg_win_hi", 62)]
    for first, last in ((5, 5), (9, 3), (-1, 4), (0, 63)):
        del seen[:]
        with pytest.raises(ZsError, match="window"):
            ops.gpt2_decode_phase_window(first=first, last=last)
        assert seen == []


def test_ops_refuse_cpu_tensors():
    import torch
    from zsaac import ops
    from zsaac._lib import ZsError
    a = torch.zeros(4, 32)
    with pytest.raises(ZsError):
        ops.gemm(a, torch.zeros(8, 32), torch.zeros(4, 8), split_k=1)
