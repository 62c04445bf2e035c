"""The SpMM shape on the CPU (sblas.spmm_shape_host: no GPU): which kernels
every named case of the GPU tests runs, and every threshold of the plan build
and of a launch at its boundary.  Expected values are written from the rules
documented in include/sblas.h, not read back from the library."""
import numpy as np
import pytest

from spmm_cases import (CASES, FORM_KERNELS, FORM_OPTS, K_NONDIRECT, K_UNSUPPORTED, PLAN_KEYS, case_shape,
                        spmm_case, spmm_matrix)
from transpose_cases import rand_csr


@pytest.fixture(scope="module")
def cases():
    return {name: spmm_case(name) for name in CASES}


def shape(sb, c, n_plan, **call):
    with sb.test_options(**c["opts"]):
        return sb.spmm_shape_host(c["k"], c["rp"], c["col"], n_plan, **call)


@pytest.mark.parametrize("n", [1, 16, 64, 100])
@pytest.mark.parametrize("name", CASES)
def test_case_shape(sb, cases, name, n):
    """the whole dict of every named case: plan built and called at width n,
    B row-major, packed and aligned, beta != 0"""
    c = cases[name]
    want = case_shape(name, c, n)
    want.update(fast=int(want["ctile"] and n % 16 == 0 and c["k"] * n * 8 < 2 ** 32), transposes_B=0, kbeta=1)
    assert shape(sb, c, n) == want


def test_case_constructions(cases):
    """what the GPU tests rely on in the named matrices"""
    c = cases["splitk_mfma"]
    assert c["m"] == 68 and 20 * 300 >= 256 * 20
    for name in ("dup_rowwave", "dup_splitk", "dup_mfma", "dup_ct"):
        c = cases[name]
        rp, col = c["rp"], c["col"]
        dups = sum(len(col[rp[r]:rp[r + 1]]) - len(np.unique(col[rp[r]:rp[r + 1]])) for r in range(c["m"]))
        assert 0.08 * rp[-1] <= dups <= 0.8 * rp[-1]
        assert any(np.any(np.diff(col[rp[r]:rp[r + 1]]) < 0) for r in range(c["m"]))  # unsorted rows
    c = cases["dup_mfma"]  # block 0 is dense only through its duplicates
    blk = c["col"][:c["rp"][16]]
    assert len(blk) == 64 and len(np.unique(blk)) == 16 and 64 >= 0.08 * 16 * 16 > 16
    c = cases["nondirect"]
    slabs = np.unique(c["col"] >> 11)
    assert set(slabs % 8) == set(range(8)) and {0, 1025, 1026} <= set(slabs)
    assert c["col"].min() == 0 and c["col"].max() == c["k"] - 1 == K_NONDIRECT - 1
    assert 25_000 <= c["rp"][-1] <= 35_000 and len(np.unique(c["col"])) < c["rp"][-1] // 5
    c = cases["empty_tail"]
    assert np.all(np.diff(c["rp"])[-40:] == 0) and c["m"] == 140


@pytest.mark.parametrize("form", ["rowwave", "splitk", "ct", "ctrows"])
@pytest.mark.parametrize("ncols", [1, 16, 64, 100])
@pytest.mark.parametrize("layout", [0, 1])
def test_test_spmm_forms(sb, ncols, layout, form):
    """the kernels every parameter set of test_kernels_gpu.test_spmm runs"""
    m, k, rp, col, val = spmm_matrix(form, np.random.default_rng(ncols + 10 * layout))
    with sb.test_options(**FORM_OPTS[form]):
        T = sb.spmm_shape_host(k, rp, col, ncols, b_layout=layout)
    assert (T["rowform"], T["ctile"], T["nmfma"]) == FORM_KERNELS[form]
    assert T["transposes_B"] == (layout == 0)
    if form == "splitk":  # without the option all 4 blocks are dense: no row kernel runs at all
        T = sb.spmm_shape_host(k, rp, col, ncols)
        assert (T["nmfma"], T["nsparse"], T["rowform"]) == (4, 0, 0)


def test_two_handles_matrices(sb):
    for i, m in enumerate((900, 1300)):
        rp, col, _ = rand_csr(np.random.default_rng(50 + i), m, 6000, 60)
        with sb.test_options(spmm_ctile=1):
            T = sb.spmm_shape_host(6000, rp, col, 64)
        assert (T["rowform"], T["ctile"], T["nmfma"], T["fast"]) == (0, 1, 0, 1)


# ------------------------------------------------------------ boundaries ----
def fill_block(nz):
    """16 rows over 25 distinct columns, two entries per row (nz <= 32)"""
    cols = np.arange(32) % 25
    lens = np.full(16, 2)
    lens[15] -= 32 - nz
    rp = np.concatenate([[0], np.cumsum(lens)])
    return rp, cols[:nz].astype(np.int32)


def test_fill_threshold(sb):
    """dense when nz >= 0.08 * 16 * |U|: |U| = 25 gives exactly 32"""
    rp, col = fill_block(32)
    assert len(np.unique(col)) == 25
    T = sb.spmm_shape_host(100, rp, col, 16)
    assert (T["nmfma"], T["nsparse"], T["sparse_nnz"], T["rowform"]) == (1, 0, 0, 0)
    rp, col = fill_block(31)
    assert len(np.unique(col)) == 25
    T = sb.spmm_shape_host(100, rp, col, 16)
    assert (T["nmfma"], T["nsparse"], T["sparse_nnz"], T["rowform"]) == (0, 16, 31, 1)
    with sb.test_options(spmm_mfma_fill=2):  # a threshold above 1: no block is dense
        rp, col = fill_block(32)
        assert sb.spmm_shape_host(100, rp, col, 16)["nmfma"] == 0
    with sb.test_options(spmm_mfma_fill=0):  # every block with an entry is
        assert sb.spmm_shape_host(100, rp, col, 16)["nmfma"] == 1
        assert sb.spmm_shape_host(100, np.zeros(17, np.int64), np.zeros(0, np.int32), 16)["nmfma"] == 0


@pytest.mark.parametrize("last,rowform", [(168, 2), (167, 1)])
def test_splitk_threshold(sb, last, rowform):
    """split-k when sparse_nnz >= 256 * nsparse: 3 rows, 768 entries, and one less"""
    lens = np.array([300, 300, last])
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.arange(L) for L in lens]).astype(np.int32)
    with sb.test_options(spmm_mfma_fill=2):
        T = sb.spmm_shape_host(5000, rp, col, 16)
    assert (T["nsparse"], T["sparse_nnz"], T["rowform"]) == (3, 600 + last, rowform)


def tiny(m, k, cols=None):
    """m rows, ~10 entries in all (one per row in the first rows), columns up to k - 1"""
    cols = np.array([0, 1, 2047, 2048, 4097, k // 2, k - 2050, k - 3, k - 2, k - 1] if cols is None else cols)
    cols = np.unique(np.clip(cols, 0, k - 1))
    lens = np.zeros(m, np.int64)
    if m >= len(cols):
        lens[:len(cols)] = 1
    else:
        lens[0] = len(cols)
    return np.concatenate([[0], np.cumsum(lens)]), cols.astype(np.int32)


@pytest.mark.parametrize("ldb,addr,n,fast", [(16, 0, 16, 1), (17, 0, 16, 0), (18, 0, 16, 1), (18, 8, 16, 0),
                                              (18, 16, 16, 1), (40, 0, 40, 0), (32, 0, 32, 1), (2, 0, 1, 0),
                                              (32, 0, 15, 0), (32, 0, 17, 0)])
def test_fast_predicate(sb, ldb, addr, n, fast):
    """row stride even, n % 16 == 0, B 16-byte aligned"""
    rp, col = tiny(700, 5000)
    with sb.test_options(spmm_ctile=1):
        T = sb.spmm_shape_host(5000, rp, col, 16, ncols=n, ldb=ldb, b_layout=1, b_addr=0x7F0000001000 + addr)
        assert (T["ctile"], T["fast"]) == (1, fast)
        # column-major: the handle's own panel, stride n, aligned whatever B's address is
        T = sb.spmm_shape_host(5000, rp, col, 16, ncols=n, ldb=5000 + ldb, b_layout=0, b_addr=0x7F0000001000 + addr)
        assert (T["transposes_B"], T["fast"]) == (1, int(n % 16 == 0))
    # the row forms have no fast kernel
    assert sb.spmm_shape_host(5000, rp, col, 16, ncols=n, ldb=ldb)["fast"] == 0


def test_kbeta(sb):
    rp, col = tiny(700, 5000)
    assert sb.spmm_shape_host(5000, rp, col, 16, beta=0.0)["kbeta"] == 0
    assert sb.spmm_shape_host(5000, rp, col, 16, beta=-0.0)["kbeta"] == 0
    assert sb.spmm_shape_host(5000, rp, col, 16, beta=1e-300)["kbeta"] == 1


@pytest.mark.parametrize("m,k,ctile", [(16384, 1 << 17, 1), (16385, 1 << 17, 0), (16384, (1 << 17) - 1, 0),
                                        (1, 1 << 17, 1), (700, 5000, 0)])
def test_default_ctile_rule(sb, m, k, ctile):
    """without the option: m <= 16384 and k >= 2^17 (and no MFMA block)"""
    rp, col = tiny(m, k)
    T = sb.spmm_shape_host(k, rp, col, 16)
    assert T["nmfma"] == 0 and T["ctile"] == ctile and T["rowform"] == 1 - ctile
    if (m, ctile) == (16384, 1):  # ceil(16384 / 1204) = 14 row blocks of ceil(16384 / 14) = 1171 rows
        assert (T["ns"], T["nrb"], T["R"], T["rbits"], T["wlog"], T["direct"]) == (2, 14, 1171, 11, 11, 1)
    with sb.test_options(spmm_ctile=0):
        assert sb.spmm_shape_host(k, rp, col, 16)["ctile"] == 0
    with sb.test_options(spmm_ctile=1):
        assert sb.spmm_shape_host(k, rp, col, 16)["ctile"] == 1


def test_ctile_needs_no_mfma_block(sb):
    rp, col = fill_block(32)
    with sb.test_options(spmm_ctile=1):
        T = sb.spmm_shape_host(100, rp, col, 16)
        assert (T["nmfma"], T["ctile"], T["ct_supported"]) == (1, 0, 1)
        T = sb.spmm_shape_host(100, np.zeros(1, np.int64), np.zeros(0, np.int32), 16)  # m = 0
        assert (T["ctile"], T["ct_supported"], T["rowform"]) == (0, 0, 0)


@pytest.mark.parametrize("m,nrb,R,rbits", [(1, 1, 1, 1), (2, 1, 2, 1), (3, 1, 3, 2), (1024, 1, 1024, 10),
                                            (1025, 1, 1025, 11), (1204, 1, 1204, 11), (1205, 2, 603, 10),
                                            (2408, 2, 1204, 11), (2409, 3, 803, 10)])
@pytest.mark.parametrize("n,ncg", [(1, 1), (16, 1), (17, 2), (64, 4), (100, 7), (600, 38)])
def test_ctile_layout_sizes(sb, m, nrb, R, rbits, n, ncg):
    """row blocks of at most 1204 rows, rbits = ceil(log2 R) (at least 1), ns = 32 / (nrb * ncg) (at least 1)"""
    rp, col = tiny(m, 5000)
    with sb.test_options(spmm_ctile=1):
        T = sb.spmm_shape_host(5000, rp, col, n)
    assert (T["ctile"], T["nrb"], T["R"], T["rbits"], T["wlog"]) == (1, nrb, R, rbits, 11)
    assert T["ns"] == max(1, 32 // (nrb * ncg))


@pytest.mark.parametrize("k,ldb,n,fast", [(17895697, 30, 16, 1),        # k * ldb * 8 = 2^32 - 16
                                           ((1 << 29) - 1, 1, 1, 0),    # 2^32 - 8: an odd stride, never fast
                                           (1 << 24, 32, 16, 0),        # 2^32
                                           (1 << 24, 32, 32, 0),
                                           ((1 << 24) - 1, 32, 32, 1),  # 2^32 - 256
                                           (K_NONDIRECT, 256, 16, 0),   # the GPU test's 4.3 GB B
                                           (K_NONDIRECT, 254, 16, 1)])
def test_offset_guard(sb, k, ldb, n, fast):
    """fast needs k * ldb * 8 < 2^32 (32-bit byte offsets); 2 rows, so rbits = 1 and every k here is
    supported and direct"""
    assert (k * ldb * 8 < 2 ** 32) == bool(fast) or ldb % 2
    rp, col = tiny(2, k)
    with sb.test_options(spmm_ctile=1):
        T = sb.spmm_shape_host(k, rp, col, 16, ncols=n, ldb=ldb)
    assert (T["ctile"], T["ct_supported"], T["rbits"], T["direct"], T["fast"]) == (1, 1, 1, 1, fast)


@pytest.mark.parametrize("k,direct", [(1 << 21, 1), ((1 << 21) + 1, 0), (K_NONDIRECT, 0)])
def test_direct_key_limit(sb, k, direct):
    """m = 1,100: rbits = 11, so keys hold the global column up to k = 2^21"""
    rp, col = tiny(1100, k)
    with sb.test_options(spmm_ctile=1):
        T = sb.spmm_shape_host(k, rp, col, 16)
    assert (T["ctile"], T["ct_supported"], T["rbits"], T["direct"]) == (1, 1, 11, direct)
    with sb.test_options(spmm_ctile=1):  # m = 1,024: rbits = 10, the limit doubles
        T = sb.spmm_shape_host(k, *tiny(1024, k), 16)
    assert (T["rbits"], T["direct"]) == (10, 1)


@pytest.mark.parametrize("k,supported", [(1 << 24, 1),                 # 8192 slabs: 1024 per XCD = 2^21 columns
                                          (8184 * 2048 + 1, 1),        # 8185 slabs: still 1024 per XCD
                                          ((1 << 24) + 1, 0),          # one slab more: 1025 per XCD
                                          (K_UNSUPPORTED, 0)])
def test_key_capacity(sb, k, supported):
    """m = 1,100 (rbits 11): XCD-local columns, ceil(slabs / 8) * 2048, must not exceed 2^21"""
    rp, col = tiny(1100, k)
    with sb.test_options(spmm_ctile=1):
        T = sb.spmm_shape_host(k, rp, col, 1)
    assert (T["ct_supported"], T["ctile"], T["rowform"]) == (supported, supported, 1 - supported)
    assert T["direct"] == 0 and T["rbits"] == (11 if supported else 0)
    T = sb.spmm_shape_host(k, rp, col, 1)  # the default rule takes the same fallback
    assert (T["ct_supported"], T["ctile"]) == (supported, supported)


def test_bucket_case_shape(sb):
    """the exact-bucket GPU test: columns below 2,048 in one row block are one slab (wlog 11) of
    XCD 0, and its first set"""
    rp, col = tiny(700, 5000, cols=[0, 5, 2047])
    with sb.test_options(spmm_ctile=1):
        T = sb.spmm_shape_host(5000, rp, col, 16)
    assert (T["wlog"], T["nrb"], T["ns"]) == (11, 1, 32) and col.max() >> T["wlog"] == 0


def test_rejects_bad_arguments(sb):
    rp, col = tiny(4, 100)
    for bad in (dict(ncols=-1), dict(b_layout=2)):
        with pytest.raises(sb.SblasError):
            sb.spmm_shape_host(100, rp, col, 16, **bad)
    with pytest.raises(sb.SblasError):
        sb.spmm_shape_host(100, rp[::-1].copy(), col, 16)
    with pytest.raises(sb.SblasError):
        sb.spmm_shape_host(-1, rp, col, 16)
    assert set(PLAN_KEYS) | {"fast", "transposes_B", "kbeta"} == set(sb.SPMM_SHAPE_KEYS)
