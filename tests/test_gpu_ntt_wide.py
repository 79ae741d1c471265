"""The NTT / LDE layer where the rest of the suite never goes: above 2^24
rows, the recurrence outer-twiddle branch, and the instantiations and launch
splits the other files' lists skip.

A. 2^25 and 2^26 rows against the oracle: the first sizes with four passes
   (split_radix gives (6,6,6,7) and (6,6,7,7), the second with two middle
   digits of different widths in the last pass's mixed-radix reversal) and
   with a first pass over blocks above 2^24, which has no outer-twiddle table
   and computes its twiddles by recurrence.  The 3-pass LDE's largest
   instantiation (2^24 -> 2^25) against the oracle on both LDE paths.
B. The documented maximum, 2^27 and 2^28 rows, on the device only: dense
   round trips, and sparse inputs against closed forms in Python integers
   that share no code with the GPU or the oracle:
     x = sum_i a_i delta_{j_i}  ->  NTT(x)[k] = sum_i a_i w^(j_i k mod n)
     (the inverse: w^-1 and a final 1/n), and for the LDE
     out[i] = sum_j a_j L_j(7 w_e^i),  L_j(X) = (w_n^j / n) (X^n - 1) / (X - w_n^j)
   (the denominator never vanishes: 7 is not in the subgroup).  One bit past
   the maximum is refused before anything is launched.
C. ZKGPU_NTT_OTW=0 sends every non-last pass down the recurrence branch, so
   radices 2^5..2^8 run it in first and middle passes at small sizes, against
   the oracle; the profiler's kernel names (",rec") prove which branch ran.
D. The sizes test_gpu_parity.py's lists skip, the 65535-column launch split
   of k_ntt_small, and zkgpu_scale_by_powers_dev against Python integers.

Not covered, because it cannot be reached: dispatch_pass `case 4` (radix 2^4).
split_radix only yields radices 2^5..2^8 for 13 <= log2 n <= 28, and smaller
transforms take k_ntt_small.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
ERR_ARG = -2  # ZKGPU_ERR_ARG (include/zkgpu.h)
SENTINEL = 0x5EED5EED5EED5EED  # fills the padding words the library must not touch


def rand_gl(rng, shape, noncanon=False):
    x = (rng.integers(0, 2**63, size=shape, dtype=np.uint64) * np.uint64(2) +
         rng.integers(0, 2, size=shape, dtype=np.uint64))
    if not noncanon:
        x %= np.uint64(P)
    return x


def rand_cols(torch, ncols, n, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return torch.randint(0, 2**63 - 1, (ncols, n), dtype=torch.int64, device="cuda:0", generator=g)


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    """hand the large tensors' memory back when the module is done"""
    yield
    import torch
    torch.cuda.empty_cache()


@pytest.fixture
def prof(zkgpu):
    """live profiling on, records empty; off and empty again afterwards"""
    zkgpu.prof_reset()
    zkgpu.prof_enable(True)
    yield zkgpu
    zkgpu.prof_enable(False)
    zkgpu.prof_reset()


def rec_names(names):
    return [k for k in names if k.endswith(",rec>")]


# ------------------------------------------------------------------ closed forms
def sparse_terms(n, seed):
    """8 non-zero entries: positions 1, n-1, n/2, n/2+1 and four random ones,
    coefficients P-1, 1 and six random canonical values"""
    rng = np.random.default_rng(seed)
    pos = [1, n - 1, n // 2, n // 2 + 1]
    while len(pos) < 8:
        j = int(rng.integers(0, n))
        if j not in pos:
            pos.append(j)
    coef = [P - 1, 1] + [int(v) for v in rng.integers(0, P, 6, dtype=np.uint64)]
    return pos, coef


def put_sparse(torch, col, pos, coef):
    col.zero_()
    vals = torch.from_numpy(np.array(coef, np.uint64).view(np.int64)).to("cuda:0")
    col[torch.tensor(pos, dtype=torch.int64, device="cuda:0")] = vals


def sample_rows(n, seed, total=2048):
    """0, 1, n-1, every 2^b and 2^b +- 1, and random rows up to `total`"""
    rows = {0, 1, n - 1}
    b = 1
    while b < n:
        rows.update(r for r in (b - 1, b, b + 1) if 0 <= r < n)
        b <<= 1
    rng = np.random.default_rng(seed)
    while len(rows) < min(total, n):
        rows.add(int(rng.integers(0, n)))
    return sorted(rows)


def gather(zkgpu, torch, col, rows):
    """the sampled rows of one device column, as Python integers"""
    idx = torch.tensor(rows, dtype=torch.int64, device="cuda:0")
    return [int(v) for v in zkgpu.from_device(col[idx])]


def ntt_closed(oracle, logn, pos, coef, rows, inverse):
    n = 1 << logn
    w = oracle.gl_w(logn)
    scale = 1
    if inverse:
        w = pow(w, -1, P)
        scale = pow(n, -1, P)
    return [scale * sum(a * pow(w, (j * k) % n, P) for j, a in zip(pos, coef)) % P for k in rows]


def lde_closed(oracle, logn, loge, pos, coef, rows):
    n, ne = 1 << logn, 1 << loge
    wn, we = oracle.gl_w(logn), oracle.gl_w(loge)
    ninv = pow(n, -1, P)
    wj = [pow(wn, j, P) for j in pos]
    s7n = pow(7, n, P)
    out = []
    for i in rows:
        x = 7 * pow(we, i, P) % P
        z = (s7n * pow(we, (i * n) % ne, P) - 1) % P  # X^n - 1
        out.append(sum(a * w * ninv % P * z % P * pow((x - w) % P, -1, P) for a, w in zip(coef, wj)) % P)
    return out


def test_closed_forms_vs_oracle(oracle):
    """the two closed forms themselves, against the oracle at a small size"""
    logn = 10
    n = 1 << logn
    pos, coef = sparse_terms(n, 1)
    x = np.zeros(n, np.uint64)
    x[pos] = np.array(coef, np.uint64)
    rows = list(range(n))
    for inv in (False, True):
        assert ntt_closed(oracle, logn, pos, coef, rows, inv) == [int(v) for v in oracle.ntt(x, inv)]
    rows = list(range(2 * n))
    assert lde_closed(oracle, logn, logn + 1, pos, coef, rows) == [int(v) for v in oracle.extend_pol(x, 2 * n)]


# ------------------------------------------------------------------ A: four passes against the oracle
@pytest.mark.parametrize("inverse", [False, True])
def test_ntt_2p25_vs_oracle(oracle, zkgpu, inverse):
    """(6,6,6,7): four passes, the first over blocks of 2^25 (no table);
    padded leading dimensions, the padding untouched"""
    import torch
    n, C = 1 << 25, 2
    ld_src, ld_dst = n + 64, n + 128
    src = rand_cols(torch, C, ld_src, 25)
    dst = torch.full((C, ld_dst), SENTINEL, dtype=torch.int64, device="cuda:0")
    zkgpu.ntt_dev(dst, ld_dst, src, ld_src, n, C, inverse=inverse)
    torch.cuda.synchronize()
    assert bool((dst[:, n:] == SENTINEL).all())
    for c in range(C):
        ref = oracle.ntt(zkgpu.from_device(src[c, :n]), inverse)
        assert np.array_equal(zkgpu.from_device(dst[c, :n]), ref), c


def test_ntt_2p26_vs_oracle_and_roundtrip(oracle, zkgpu):
    """(6,6,7,7): the last pass's two middle digits have different widths"""
    import torch
    n = 1 << 26
    x = rand_cols(torch, 1, n, 26)
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    zkgpu.ntt_dev(y, n, x, n, n, 1, inverse=False)
    zkgpu.ntt_dev(z, n, y, n, n, 1, inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(z, x)
    assert np.array_equal(zkgpu.from_device(y[0]), oracle.ntt(zkgpu.from_device(x[0])))


def test_large_first_pass_is_recurrence(prof):
    """what ran, from the profiler's names: the first pass of a 2^25
    transform has no table, every pass of a 2^20 transform has one"""
    import torch
    zkgpu = prof
    n = 1 << 25
    x = rand_cols(torch, 1, n, 3)
    y = torch.empty_like(x)
    zkgpu.ntt_dev(y, n, x, n, n, 1, inverse=False)
    assert zkgpu.prof_kernels() == ["k_ntt_pass<6,fwd,rec>", "k_ntt_pass<6,fwd>", "k_ntt_pass<7,fwd>"]
    assert zkgpu.prof_query("k_ntt_pass<6,fwd,rec>")[0] == 1
    assert zkgpu.prof_query("k_ntt_pass<6,fwd>")[0] == 2
    assert zkgpu.prof_query("k_ntt_pass<7,fwd>")[0] == 1
    zkgpu.prof_reset()
    zkgpu.ntt_dev(y, n, x, n, n, 1, inverse=True)
    assert zkgpu.prof_kernels() == ["k_ntt_pass<6,inv,rec>", "k_ntt_pass<6,inv>", "k_ntt_pass<7,inv>"]
    zkgpu.prof_reset()
    n = 1 << 20
    for inv in (False, True):
        zkgpu.ntt_dev(y, n, x, n, n, 1, inverse=inv)
    names = zkgpu.prof_kernels()
    assert sorted(names) == ["k_ntt_pass<6,fwd>", "k_ntt_pass<6,inv>", "k_ntt_pass<7,fwd>", "k_ntt_pass<7,inv>"]
    assert rec_names(names) == []


@pytest.fixture(scope="module")
def lde_2p24(oracle, zkgpu):
    """one column of 2^24 rows in a padded buffer, and its oracle extension"""
    import torch
    n = 1 << 24
    src = rand_cols(torch, 1, n + 64, 24)
    ref = oracle.extend_pol(zkgpu.from_device(src[0, :n]), 2 * n)
    ref.setflags(write=False)
    return src, ref


@pytest.mark.parametrize("lde3", ["0", "1"])
def test_lde_2p24_vs_oracle(prof, lde_2p24, lde3, monkeypatch):
    """2^24 -> 2^25 on both LDE paths: the 3-pass LDE's largest instantiation
    (k_lde_strided<12>, k_lde_mid with RA = 4096, outer tables of 2^24
    entries), and the 6-pass chain whose forward transform has four passes"""
    import torch
    zkgpu = prof
    monkeypatch.setenv("ZKGPU_LDE3", lde3)
    src, ref = lde_2p24
    n, ne = 1 << 24, 1 << 25
    ld_in, ld_out = n + 64, ne + 128
    out = torch.full((1, ld_out), SENTINEL, dtype=torch.int64, device="cuda:0")
    zkgpu.extend_pol_dev(out, ld_out, src, ld_in, ne, n, 1)
    torch.cuda.synchronize()
    names = zkgpu.prof_kernels()
    if lde3 == "1":
        assert names == ["k_lde_p1<12>", "k_lde_mid", "k_lde_p3<12>"]
    else:
        assert "k_ntt_pass<6,fwd,rec>" in names and not any(k.startswith("k_lde") for k in names)
    assert bool((out[:, ne:] == SENTINEL).all())
    assert np.array_equal(zkgpu.from_device(out[0, :ne]), ref)


# ------------------------------------------------------------------ B: the documented maximum
@pytest.mark.parametrize("logn,ncols", [(27, 2), (28, 1)])
def test_ntt_max_roundtrip_and_sparse(oracle, zkgpu, logn, ncols):
    """(6,7,7,7) and (7,7,7,7): INTT(NTT(x)) == x on dense data, and sparse
    inputs against the closed form at the sampled rows, both directions"""
    import torch
    n = 1 << logn
    x = rand_cols(torch, ncols, n, logn)
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    zkgpu.ntt_dev(y, n, x, n, n, ncols, inverse=False)
    zkgpu.ntt_dev(z, n, y, n, n, ncols, inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(z, x)
    del z
    terms = [sparse_terms(n, 100 * logn + c) for c in range(ncols)]
    for c, (pos, coef) in enumerate(terms):
        put_sparse(torch, x[c], pos, coef)
    rows = sample_rows(n, logn)
    for inv in (False, True):
        zkgpu.ntt_dev(y, n, x, n, n, ncols, inverse=inv)
        torch.cuda.synchronize()
        for c, (pos, coef) in enumerate(terms):
            got = gather(zkgpu, torch, y[c], rows)
            want = ntt_closed(oracle, logn, pos, coef, rows, inv)
            bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
            assert not bad, (inv, c, len(bad), bad[:4])


def test_lde_max_sparse_and_coefficients(oracle, zkgpu, monkeypatch):
    """2^27 -> 2^28, the default LDE path: a sparse input against the closed
    form, and for a dense x the output's coefficients c = INTT(out): c[n:]
    is zero and NTT_n(c[k] 7^-k) gives x back"""
    import torch
    monkeypatch.delenv("ZKGPU_LDE3", raising=False)
    logn, loge = 27, 28
    n, ne = 1 << logn, 1 << loge
    x = torch.empty((1, n), dtype=torch.int64, device="cuda:0")
    out = torch.empty((1, ne), dtype=torch.int64, device="cuda:0")
    pos, coef = sparse_terms(n, 2728)
    put_sparse(torch, x[0], pos, coef)
    zkgpu.extend_pol_dev(out, ne, x, n, ne, n, 1)
    torch.cuda.synchronize()
    rows = sample_rows(ne, 28)
    got = gather(zkgpu, torch, out[0], rows)
    want = lde_closed(oracle, logn, loge, pos, coef, rows)
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert not bad, (len(bad), bad[:4])

    x = rand_cols(torch, 1, n, 2728)
    zkgpu.extend_pol_dev(out, ne, x, n, ne, n, 1)
    c = torch.empty_like(out)
    zkgpu.ntt_dev(c, ne, out, ne, ne, 1, inverse=True)
    torch.cuda.synchronize()
    assert not bool(c[0, n:].any())
    zkgpu.scale_by_powers_dev(c, ne, 1, n, pow(7, -1, P))
    back = torch.empty_like(x)
    zkgpu.ntt_dev(back, n, c, ne, n, 1, inverse=False)
    torch.cuda.synchronize()
    assert torch.equal(back, x)


def test_one_bit_past_the_maximum_is_refused(prof):
    """2^29 rows: ZKGPU_ERR_ARG before anything is launched (the tiny buffer
    is never dereferenced)"""
    import torch
    zkgpu = prof
    L = zkgpu.lib()
    t = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    big = 1 << 29
    for inv in (0, 1):
        assert L.zkgpu_gl_ntt_dev(t.data_ptr(), big, t.data_ptr(), big, big, 1, inv) == ERR_ARG
    assert L.zkgpu_gl_extend_pol_dev(t.data_ptr(), big, t.data_ptr(), big >> 1, big, big >> 1, 1) == ERR_ARG
    assert L.zkgpu_gl_extend_pol_dev(t.data_ptr(), big, t.data_ptr(), 16, big, 16, 1) == ERR_ARG
    with pytest.raises(zkgpu.ZkgpuError):
        zkgpu.ntt_dev(t, big, t, big, big, 1)
    torch.cuda.synchronize()
    assert zkgpu.prof_kernels() == []
    assert not bool(t.any())


# ------------------------------------------------------------------ C: the recurrence branch at small sizes
def _with_and_without_tables(zkgpu, monkeypatch, run, ref):
    """run() under ZKGPU_NTT_OTW=0 (a ,rec pass must have run) and with the
    variable unset (none may), both equal to ref"""
    monkeypatch.setenv("ZKGPU_NTT_OTW", "0")
    zkgpu.prof_reset()
    got = run()
    assert rec_names(zkgpu.prof_kernels()), zkgpu.prof_kernels()
    assert np.array_equal(got, ref)
    monkeypatch.delenv("ZKGPU_NTT_OTW")
    zkgpu.prof_reset()
    got = run()
    names = zkgpu.prof_kernels()
    assert names and not rec_names(names), names
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("logn,ncols,noncanon", [(13, 2, False), (15, 2, False), (16, 2, False), (17, 3, False),
                                                 (17, 3, True), (21, 1, False)])
def test_ntt_recurrence_twiddles_vs_oracle(oracle, prof, logn, ncols, noncanon, monkeypatch):
    """splits (6,7), (7,8), (8,8), (5,6,6), (7,7,7): radices 2^5..2^8 in a
    non-last pass, a middle pass included"""
    zkgpu = prof
    rng = np.random.default_rng(1300 + logn + noncanon)
    x = rand_gl(rng, (1 << logn, ncols), noncanon=noncanon)
    for inv in (False, True):
        _with_and_without_tables(zkgpu, monkeypatch, lambda: zkgpu.ntt(x, inv), oracle.ntt(x, inv))


@pytest.mark.parametrize("logn,blow,ncols", [(16, 1, 3), (14, 2, 2)])
def test_extend_pol_recurrence_twiddles_vs_oracle(oracle, prof, logn, blow, ncols, monkeypatch):
    """the 6-pass chain with recurrence twiddles: the zero-padded forward
    transform (blowup 1: half_zero set in its first pass)"""
    zkgpu = prof
    monkeypatch.setenv("ZKGPU_LDE3", "0")
    rng = np.random.default_rng(1400 + logn)
    x = rand_gl(rng, (1 << logn, ncols))
    ne = 1 << (logn + blow)
    _with_and_without_tables(zkgpu, monkeypatch, lambda: zkgpu.extend_pol(x, ne), oracle.extend_pol(x, ne))


def test_other_values_keep_the_tables(prof, monkeypatch):
    """only ZKGPU_NTT_OTW=0 switches the tables off"""
    zkgpu = prof
    x = rand_gl(np.random.default_rng(7), (1 << 13, 1))
    for v in ("1", "", "00", "off"):
        monkeypatch.setenv("ZKGPU_NTT_OTW", v)
        zkgpu.prof_reset()
        zkgpu.ntt(x)
        assert zkgpu.prof_kernels() == ["k_ntt_pass<6,fwd>", "k_ntt_pass<7,fwd>"], v


# ------------------------------------------------------------------ D: gaps in the other files' lists
@pytest.mark.parametrize("logn,ncols", [(15, 2), (18, 2), (21, 1), (22, 1)])
def test_ntt_vs_oracle_missing_sizes(oracle, zkgpu, logn, ncols):
    """(7,8): the only two-pass size with a radix-2^7 first pass in front of a
    radix-2^8 last one; (6,6,6); (7,7,7); (7,7,8)"""
    rng = np.random.default_rng(100 + logn)
    x = rand_gl(rng, (1 << logn, ncols))
    for inv in (False, True):
        assert np.array_equal(zkgpu.ntt(x, inv), oracle.ntt(x, inv)), (logn, ncols, inv)


def test_small_ntt_65537_columns(oracle, zkgpu):
    """k_ntt_small's launches split at 65535 columns: every column, NTT both
    directions and extend_pol 2^2 -> 2^3"""
    rng = np.random.default_rng(65537)
    x = rand_gl(rng, (4, 65537))
    for inv in (False, True):
        assert np.array_equal(zkgpu.ntt(x, inv), oracle.ntt(x, inv)), inv
    assert np.array_equal(zkgpu.extend_pol(x, 8), oracle.extend_pol(x, 8))


@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("n", [1, 65, 16384, 16385, 40000])
def test_scale_by_powers_dev(zkgpu, n, ncols):
    """cols[c][k] *= base^k against Python integers (16385: the first size
    with two workgroups); non-canonical inputs, canonical outputs, the padding
    of each column untouched"""
    import torch
    rng = np.random.default_rng(n + ncols)
    ld = n + 5
    cols = rand_gl(rng, (ncols, ld), noncanon=True)
    special = [P, P + 1, 2**64 - 1, 0, P - 1, 2**32, 2**64 - 2**32]
    for i, v in enumerate(special[:n]):
        cols[i % ncols, (i * 7919) % n] = v
    cols[:, n:] = SENTINEL
    xs = [[int(v) for v in cols[c, :n]] for c in range(ncols)]
    for base in (0, 1, 7, pow(7, -1, P), P - 1, P + 2):
        d = zkgpu.to_device(cols)
        zkgpu.scale_by_powers_dev(d, ld, ncols, n, base)
        torch.cuda.synchronize()
        got = zkgpu.from_device(d)
        assert np.all(got[:, n:] == np.uint64(SENTINEL)), base
        pw, f = [], 1
        for _ in range(n):
            pw.append(f)
            f = f * base % P
        for c in range(ncols):
            want = np.array([v * q % P for v, q in zip(xs[c], pw)], dtype=np.uint64)
            bad = np.nonzero(got[c, :n] != want)[0]
            assert bad.size == 0, (base, c, bad[:4], got[c, bad[:4]], want[bad[:4]])
