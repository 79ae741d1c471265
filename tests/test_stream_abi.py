"""The streamed hand-off's entry points exist in the built libraries and in
the Python binding (no GPU): the chunked leaf sponge, the column-window
loader and zkgpu_stark_prove_from_rows."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(zkgpu_\w+)\s*\(", text))


def test_libzkgpu_exports_the_streaming_entries():
    import zkgpu
    L = ctypes.CDLL(zkgpu.LIB_PATH)
    for name in ("zkgpu_gl_merkle_leaves_absorb_dev", "zkgpu_gl_merkle_finish_dev", "zkgpu_load_rows_window_dev",
                 "zkgpu_load_stream_open", "zkgpu_load_stream_window", "zkgpu_load_stream_close"):
        assert hasattr(L, name), name
        assert name in _declared("zkgpu.h"), name
        assert name in zkgpu.exported_symbols(), name
    for f in ("merkle_leaves_absorb_dev", "merkle_finish_dev", "load_rows_window_dev", "RowsStream"):
        assert hasattr(zkgpu, f), f


def test_libzkgpu_stark_exports_prove_from_rows():
    from zkgpu import stark
    L = ctypes.CDLL(stark.STARK_LIB)
    assert hasattr(L, "zkgpu_stark_prove_from_rows")
    assert "zkgpu_stark_prove_from_rows" in _declared("zkgpu_stark.h")
    assert callable(getattr(stark.GpuStark, "prove_from_rows", None))
    assert callable(getattr(stark.GpuStark, "prove_from_rows_raw", None))
