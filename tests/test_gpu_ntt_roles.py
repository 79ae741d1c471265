"""Every instantiation of the NTT pass kernel (k_ntt_pass, csrc/ntt.hip),
bit-exact against the oracle's NTT and extendPol at the smallest shapes that
reach it, all rows.

The kernel is specialised at compile time by what a launch is:
  role   non-last pass with table outer twiddles / with recurrence outer
         twiddles (ZKGPU_NTT_OTW=0) / last pass
  input  full / exactly the upper half zero padding (first forward pass of the
         LDE n -> 2n) / any other padding (LDE n -> 4n: a compare per load)
  post   none (forward NTT) / one factor (inverse NTT: 1/n) / per-row tables
         (the LDE's last inverse pass: 7^k / n)
Sizes: 2^13 (6,7: two passes, no radix 2^8), 2^16 (8,8: a first and a last
pass, no middle), 2^17 (5,6,6: a middle pass), 2^20 (6,7,7); LDE 2^15 -> 2^16,
2^16 -> 2^17 and 2^14 -> 2^16.  Columns 1, 3, 5, 17.  Column strides n + 8,
the in-place LDE, and the recurrence path.  Inputs carry 0, p - 1 and
non-canonical words >= p beside random ones.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
SENTINEL = 0x5EED5EED5EED5EED  # padding words the library must not touch


def words(seed, n, ncols):
    """(n, ncols) 64-bit words: random (about one in 2^32 of them >= p), with
    0, p - 1, p, p + 1 and 2^64 - 1 at the first, the last and the middle
    rows of every column and at random rows"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 2**63, size=(n, ncols), dtype=np.uint64) * np.uint64(2) +
         rng.integers(0, 2, size=(n, ncols), dtype=np.uint64))
    special = np.array([0, P - 1, P, P + 1, 2**64 - 1], dtype=np.uint64)
    for c in range(ncols):
        rows = np.concatenate(([0, 1, n // 2 - 1, n // 2, n - 2, n - 1], rng.integers(0, n, 26)))
        x[rows, c] = special[(np.arange(rows.size) + c) % special.size]
    return x


def canon(a):
    return np.asarray(a, np.uint64) % np.uint64(P)


_refs = {}


def ref(oracle, kind, logn, ncols, arg):
    """(input, oracle output) of one shape, computed once and left unchanged"""
    key = (kind, logn, ncols, arg)
    if key not in _refs:
        x = words(1000 * logn + 10 * ncols + len(kind), 1 << logn, ncols)
        y = canon(oracle.ntt(x, arg) if kind == "ntt" else oracle.extend_pol(x, 1 << (logn + arg)))
        x.setflags(write=False)
        y.setflags(write=False)
        _refs[key] = (x, y)
    return _refs[key]


def to_cols(zkgpu, torch, x, ld):
    """(n, ncols) host rows -> (ncols, ld) device columns, padding = SENTINEL"""
    n, ncols = x.shape
    t = torch.full((ncols, ld), SENTINEL, dtype=torch.int64, device="cuda:0")
    t[:, :n] = zkgpu.to_device(np.ascontiguousarray(x.T))
    return t


def check_cols(zkgpu, t, want):
    """device columns (ncols, ld) against (n, ncols) rows; the padding is intact"""
    n, ncols = want.shape
    got = zkgpu.from_device(t)
    assert np.array_equal(canon(got[:, :n].T), want)
    assert np.all(got[:, n:] == np.uint64(SENTINEL))


NTT_SHAPES = [(13, 1), (13, 17), (16, 3), (16, 5), (17, 1), (17, 5), (17, 17), (20, 3)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("logn,ncols", NTT_SHAPES)
def test_ntt_roles_vs_oracle(oracle, zkgpu, logn, ncols, inverse):
    """table outer twiddles, full input; last pass without a factor (forward)
    and with the single factor 1/n (inverse)"""
    x, want = ref(oracle, "ntt", logn, ncols, inverse)
    assert np.array_equal(canon(zkgpu.ntt(x, inverse)), want)


@pytest.mark.parametrize("logn,blow,ncols", [(15, 1, 3), (15, 1, 17), (16, 1, 1), (16, 1, 5), (14, 2, 3)])
def test_lde_roles_vs_oracle(oracle, zkgpu, logn, blow, ncols, monkeypatch):
    """n -> 2n: the first forward pass loads only the non-zero half, the last
    inverse pass applies the per-row factor tables; n -> 4n: the first forward
    pass compares every row against the input's length"""
    monkeypatch.setenv("ZKGPU_LDE3", "0")
    x, want = ref(oracle, "lde", logn, ncols, blow)
    assert np.array_equal(canon(zkgpu.extend_pol(x, 1 << (logn + blow))), want)


@pytest.mark.parametrize("logn,ncols", [(13, 3), (16, 5), (17, 5), (20, 3)])
def test_ntt_roles_recurrence_vs_oracle(oracle, zkgpu, logn, ncols, monkeypatch):
    """recurrence outer twiddles in every non-last pass, both directions"""
    monkeypatch.setenv("ZKGPU_NTT_OTW", "0")
    zkgpu.prof_reset()
    zkgpu.prof_enable(True)
    try:
        for inverse in (False, True):
            x, want = ref(oracle, "ntt", logn, ncols, inverse)
            assert np.array_equal(canon(zkgpu.ntt(x, inverse)), want)
        names = zkgpu.prof_kernels()
    finally:
        zkgpu.prof_enable(False)
        zkgpu.prof_reset()
    assert any(k.endswith(",rec>") for k in names), names


@pytest.mark.parametrize("logn,blow,ncols", [(15, 1, 3), (16, 1, 5), (14, 2, 3)])
def test_lde_roles_recurrence_vs_oracle(oracle, zkgpu, logn, blow, ncols, monkeypatch):
    """the padded first forward passes (half zero, compared) with recurrence
    outer twiddles"""
    monkeypatch.setenv("ZKGPU_LDE3", "0")
    monkeypatch.setenv("ZKGPU_NTT_OTW", "0")
    x, want = ref(oracle, "lde", logn, ncols, blow)
    assert np.array_equal(canon(zkgpu.extend_pol(x, 1 << (logn + blow))), want)


@pytest.mark.parametrize("logn,ncols", [(16, 3), (17, 5)])
def test_ntt_roles_padded_columns(oracle, zkgpu, logn, ncols):
    """column stride n + 8 for source and destination, on the device"""
    import torch
    n = 1 << logn
    for inverse in (False, True):
        x, want = ref(oracle, "ntt", logn, ncols, inverse)
        src = to_cols(zkgpu, torch, x, n + 8)
        dst = torch.full((ncols, n + 8), SENTINEL, dtype=torch.int64, device="cuda:0")
        zkgpu.ntt_dev(dst, n + 8, src, n + 8, n, ncols, inverse=inverse)
        torch.cuda.synchronize()
        check_cols(zkgpu, dst, want)
        check_cols(zkgpu, src, canon(x))


@pytest.mark.parametrize("logn,ncols", [(15, 3), (16, 5)])
def test_lde_roles_padded_columns_and_inplace(oracle, zkgpu, logn, ncols, monkeypatch):
    """extendPol n -> 2n with column strides n + 8 / 2n + 8, and in place"""
    import torch
    monkeypatch.setenv("ZKGPU_LDE3", "0")
    n, ne = 1 << logn, 2 << logn
    x, want = ref(oracle, "lde", logn, ncols, 1)
    src = to_cols(zkgpu, torch, x, n + 8)
    out = torch.full((ncols, ne + 8), SENTINEL, dtype=torch.int64, device="cuda:0")
    zkgpu.extend_pol_dev(out, ne + 8, src, n + 8, ne, n, ncols)
    torch.cuda.synchronize()
    check_cols(zkgpu, out, want)

    base = torch.full((ncols * ne + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    base[:ncols * n] = zkgpu.to_device(np.ascontiguousarray(x.T)).reshape(-1)
    zkgpu.extend_pol_inplace_dev(base, ne, n, ncols)
    torch.cuda.synchronize()
    got = zkgpu.from_device(base)
    assert np.array_equal(canon(got[:ncols * ne].reshape(ncols, ne).T), want)
    assert np.all(got[ncols * ne:] == np.uint64(SENTINEL))
