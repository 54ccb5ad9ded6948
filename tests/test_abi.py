"""The C-ABI libraries load and export every entry point their headers declare,
and the product path fails loudly without a GPU (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
PKG = ROOT / "path-tracer_amd"


def declared_functions(header: Path, prefix: str):
    text = header.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    names = re.findall(r"\b(" + prefix + r"[A-Z]\w*)\s*\(", text)
    return sorted(set(names))


@pytest.mark.parametrize("header,lib,prefix", [
    ("pt_api.h", "libpathtracer.so", "pt"),
    ("pt_scene.h", "libptscene.so", "pts"),
])
def test_library_exports_every_declared_symbol(header, lib, prefix):
    names = declared_functions(INCLUDE / header, prefix)
    if prefix == "pt":
        names = [n for n in names if not n.startswith("pts")]
    assert len(names) >= 10
    L = C.CDLL(str(PKG / lib))
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, f"{lib} lacks {missing}"


def test_python_bindings_cover_headers(pt):
    N = pt._native
    api = set(declared_functions(INCLUDE / "pt_api.h", "pt")) - set(declared_functions(INCLUDE / "pt_scene.h", "pts"))
    assert api <= set(N.HIP_API), api - set(N.HIP_API)
    assert set(declared_functions(INCLUDE / "pt_scene.h", "pts")) <= set(N.SCENE_API)


def test_struct_layouts(pt):
    N = pt._native
    assert N.HIT_RECORD_DTYPE.itemsize == 24
    assert N.PIXEL_STATE_DTYPE.itemsize == 96
    assert C.sizeof(N.pt_basic_renderer_params) == 20
    assert N.SHAPE_DTYPE.itemsize == 144 and N.CAMERA_DTYPE.itemsize == 160


def test_product_path_fails_loudly_without_gpu(pt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert pt.device_count() == 0
    with pytest.raises(pt.PathTracerError):
        pt.Device(0)


def test_missing_extension_raises(pt, monkeypatch):
    N = pt._native
    monkeypatch.setattr(N, "_hip_lib", None)
    monkeypatch.setattr(N, "HIP_LIB_PATH", PKG / "does-not-exist.so")
    with pytest.raises(N.NativeLibraryMissing):
        N.hip_lib()


def test_null_arguments_rejected(pt):
    """Calls with NULL handles return an error status instead of crashing."""
    L = pt._native.hip_lib()
    assert L.ptSynchronize(None) != 0
    assert L.ptRunBasicRenderer(None, None, 1) != 0
    assert L.ptResetBasicRenderer(None, None) != 0
    assert L.ptCreateSampleBuffer(None, 4, 4) is None
    assert len(L.ptGetLastError()) > 0
    L.ptDestroyBasicRenderer(None, None)
    L.ptDestroySampleBuffer(None, None)
    L.ptDestroyScene(None, None)
    L.ptDestroyDevice(None)
    assert L.ptWriteBasicRendererState(None, None, None) != 0
    assert L.ptGetBasicRendererShadeInfo(None, None) != 0
    assert L.ptReadBasicRendererStreamAccumulator(None, None, 0, None) != 0
    assert L.ptSetBasicRendererSplit(None, 2) != 0
    assert L.ptGetBasicRendererSplit(None, None, None, None) != 0
    assert L.ptSetBasicRendererClassLists(None, 0) != 0
    assert L.ptGetBasicRendererClassLists(None, None) != 0
    out = np.zeros(1, dtype=pt._native.HIT_RECORD_DTYPE)
    assert L.ptTraceRays(None, None, 1, None, None, None, out.ctypes.data) != 0
    words = np.zeros(4, dtype=np.uint32)
    wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.ptEvalNumerics(None, 0, 4, wp, wp, None, wp) != 0
    assert L.ptEvalNumerics(None, 0, 0, None, None, None, None) != 0
    assert b"null" in L.ptGetLastError()
    uv = np.zeros(8, dtype=np.float32)
    fp = uv.ctypes.data_as(C.POINTER(C.c_float))
    assert L.ptSampleTextures(None, None, 2, wp, fp, 0, fp) != 0
    assert b"null" in L.ptGetLastError()
    assert L.ptEvalSlabTest(None, 1, fp, fp, fp, fp, fp, 1, wp, wp) != 0
    assert b"null" in L.ptGetLastError()
    assert L.ptSceneFastDivision(None, wp) != 0
    assert not words.any() and not uv.any()


def test_numerics_op_list_matches_header(pt):
    """_native.NUMERICS_OPS is the PT_NUM_* enum of pt_numerics.h: same names,
    same ids, and the operand / output counts of its two tables."""
    N = pt._native
    text = (INCLUDE / "pt_numerics.h").read_text()
    enum = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"\bPT_NUM_(\w+)\s*=\s*(\d+)", text))
    assert enum.pop("op_count") == len(N.NUMERICS_OPS)
    assert enum == {name: i for i, name in enumerate(N.NUMERICS_OPS)}
    assert set(N.NUMERICS_OPERANDS) | set(N.NUMERICS_OUTPUTS) | set(N.NUMERICS_DEVICE_ONLY) <= set(N.NUMERICS_OPS)


def test_oracle_batch_evaluation_contract(pt):
    """oracle_fp_eval / oracle_sample_textures: exported, every host op
    answers with the table's output count, device-only and unknown ops and
    missing operands are refused without a write."""
    import oracle_lib
    N = pt._native
    L = oracle_lib.lib()
    one = np.array([0x3F800000, 0x40000000, 0x3F000000], dtype=np.uint32)
    for name in N.NUMERICS_OPS:
        k = N.NUMERICS_OPERANDS.get(name, 1)
        if name in N.NUMERICS_DEVICE_ONLY:
            with pytest.raises(ValueError):
                oracle_lib.fp_eval(name, *([one] * k))
            continue
        got = oracle_lib.fp_eval(name, *([one] * k))
        assert got.shape == ((3,) if N.NUMERICS_OUTPUTS.get(name, 1) == 1 else (3, N.NUMERICS_OUTPUTS[name]))
        if k > 1:
            with pytest.raises(ValueError):
                oracle_lib.fp_eval(name, *([one] * (k - 1) + [None]))
    assert oracle_lib.fp_eval("add", one, one).tolist() == [0x40000000, 0x40800000, 0x3F800000]
    out = np.full(3, 0xABCDEF01, dtype=np.uint32)
    p = one.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.oracle_fp_eval(len(N.NUMERICS_OPS), 3, p, p, p, out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0
    assert L.oracle_fp_eval(0, 3, p, p, p, None) != 0
    assert np.all(out == 0xABCDEF01)
    assert L.oracle_sample_textures(None, 0, None, None, None) != 0
