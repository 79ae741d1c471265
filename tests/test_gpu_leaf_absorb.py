"""The chunked leaf sponge (zkgpu_gl_merkle_leaves_absorb_dev +
zkgpu_gl_merkle_finish_dev, csrc/poseidon.hip k_leaves_absorb): a tree built
while its section arrives in column chunks, the linear hash's capacity carried
between the launches in the tree's leaf slots, must equal the one-launch tree
(zkgpu_gl_merkletree_dev) node for node -- whatever the chunking, the copy
case (<= 4 columns, one chunk) and row counts below one workgroup included."""
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [3, 4, 5, 8, 9, 16, 13, 100, 751]


def chunkings(w):
    """the whole width; all-8s; [64, rest]; [8, rest] -- those the width
    admits (every chunk but the last a multiple of 8, <= 4 columns whole)"""
    out = {"whole": [w]}
    if w > 8:
        out["all8"] = [8] * (w // 8) + ([w % 8] if w % 8 else [])
        out["8_rest"] = [8, w - 8]
    if w > 64:
        out["64_rest"] = [64, w - 64]
    return out


CASES = [(w, name) for w in WIDTHS for name in chunkings(w)]


def _src(ncols, n, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 2**63 - 1, (ncols, n), dtype=torch.int64, device="cuda", generator=g)


def _chunked(zkgpu, src, n, chunks):
    import torch
    ncols = src.shape[0]
    # the leaf slots start as garbage: the first chunk must not read them
    got = torch.full((zkgpu.merkle_num_elements(n),), -1, dtype=torch.int64, device="cuda")
    c0 = 0
    for nc in chunks:
        zkgpu.merkle_leaves_absorb_dev(got, src[c0:], n, c0, nc, ncols, n)
        c0 += nc
    assert c0 == ncols
    zkgpu.merkle_finish_dev(got, n)
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def trees(zkgpu):
    """(source, one-launch tree) per width at 2^10 rows, built once"""
    import torch
    n = 1 << 10
    out = {}
    for w in WIDTHS:
        src = _src(w, n, w)
        ref = torch.empty(zkgpu.merkle_num_elements(n), dtype=torch.int64, device="cuda")
        zkgpu.merkletree_dev(ref, src, n, w, n)
        out[w] = (src, ref)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ncols,chunking", CASES, ids=["w%d-%s" % c for c in CASES])
def test_chunked_tree_equals_one_launch_tree(zkgpu, trees, ncols, chunking):
    import torch
    src, ref = trees[ncols]
    got = _chunked(zkgpu, src, 1 << 10, chunkings(ncols)[chunking])
    assert torch.equal(got, ref)


@pytest.mark.parametrize("n", [2, 32])
def test_small_row_counts(zkgpu, n):
    """less than one workgroup: the row guard"""
    import torch
    src = _src(100, n, 1000 + n)
    ref = torch.empty(zkgpu.merkle_num_elements(n), dtype=torch.int64, device="cuda")
    zkgpu.merkletree_dev(ref, src, n, 100, n)
    got = _chunked(zkgpu, src, n, [8, 88, 4])
    assert torch.equal(got, ref)


def test_argument_errors(zkgpu):
    import torch
    from zkgpu import ZkgpuError
    n = 1 << 4
    src = _src(24, n, 7)
    nodes = torch.zeros(zkgpu.merkle_num_elements(n), dtype=torch.int64, device="cuda")
    with pytest.raises(ZkgpuError, match="multiple of 8"):  # a misaligned col0
        zkgpu.merkle_leaves_absorb_dev(nodes, src, n, 4, 8, 24, n)
    with pytest.raises(ZkgpuError, match="only the last chunk"):  # a non-final chunk of 5 columns
        zkgpu.merkle_leaves_absorb_dev(nodes, src, n, 8, 5, 24, n)
    with pytest.raises(ZkgpuError, match="outside the section"):  # col0 + ncols > total_cols
        zkgpu.merkle_leaves_absorb_dev(nodes, src, n, 16, 16, 24, n)
    with pytest.raises(ZkgpuError, match="one chunk"):  # the copy case in two chunks
        zkgpu.merkle_leaves_absorb_dev(nodes, src, n, 0, 2, 4, n)
    with pytest.raises(ZkgpuError, match="power of two"):
        zkgpu.merkle_finish_dev(nodes, 12)
    torch.cuda.synchronize()
    assert not nodes.any()  # no refused call launched anything
