"""The column-window loader (zkgpu_load_rows_window_dev, csrc/api.hip): the
window [col0, col0 + wcols) of a host row-major buffer lands in device columns
cols + c*ld, through strided block copies and the two-half stage; the columns
outside the window and the ld padding stay untouched.  The streamed form
(zkgpu_load_stream_*) queues several windows on one lane."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NROWS, NCOLS, LD, BLOCK = 1000, 37, 1024, 96  # 96 does not divide 1000: a short last block
SENTINEL = 0x5EA15EA15EA15EA1


@pytest.fixture(scope="module")
def rows():
    return np.random.default_rng(37).integers(0, 2**64 - 1, (NROWS, NCOLS), dtype=np.uint64)


def _expect(rows, windows):
    """device image (NCOLS x LD) after loading `windows` over the sentinel"""
    want = np.full((NCOLS, LD), SENTINEL, np.uint64)
    for c0, w in windows:
        want[c0:c0 + w, :NROWS] = rows[:, c0:c0 + w].T
    return want


@pytest.mark.parametrize("register_host", [0, 1])
@pytest.mark.parametrize("col0,wcols", [(0, 37), (8, 16), (32, 5)])
def test_window_lands_in_its_columns_only(zkgpu, rows, col0, wcols, register_host):
    import torch
    src = rows.copy()  # (a buffer of the test's own to page-lock)
    dev = zkgpu.to_device(np.full((NCOLS, LD), SENTINEL, np.uint64))
    zkgpu.load_rows_window_dev(dev[col0], LD, src, col0, wcols, block_rows=BLOCK, register_host=bool(register_host))
    torch.cuda.synchronize()
    assert np.array_equal(zkgpu.from_device(dev), _expect(rows, [(col0, wcols)]))


def test_window_argument_errors(zkgpu, rows):
    from zkgpu import ZkgpuError
    dev = zkgpu.to_device(np.zeros((NCOLS, LD), np.uint64))
    with pytest.raises(ZkgpuError, match="outside the 37 columns"):
        zkgpu.load_rows_window_dev(dev, LD, rows, 32, 6)
    with pytest.raises(ZkgpuError, match="ld 999 < nrows"):
        zkgpu.load_rows_window_dev(dev, 999, rows, 0, 8)


def test_streamed_windows_share_one_lane(zkgpu, rows):
    """three windows queued back to back on one loader (a stage half of 96
    window rows of the widest: many blocks per window, the halves reused
    across the windows), read on the library stream without a host wait"""
    import torch
    dev = zkgpu.to_device(np.full((NCOLS, LD), SENTINEL, np.uint64))
    stage = torch.zeros(2 * BLOCK * 16, dtype=torch.int64, device="cuda")
    snap = torch.empty_like(dev)
    s = zkgpu.RowsStream(rows, stage)
    try:
        for c0, w in [(0, 16), (16, 16), (32, 5)]:
            s.window(dev[c0], LD, c0, w)
        zkgpu.lib().zkgpu_memcpy_d2d(snap.data_ptr(), dev.data_ptr(), NCOLS * LD * 8)  # ordered after the windows
    finally:
        s.close()
    torch.cuda.synchronize()
    assert np.array_equal(zkgpu.from_device(snap), _expect(rows, [(0, 37)]))
