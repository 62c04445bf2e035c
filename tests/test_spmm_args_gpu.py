"""SpMM at the arguments the kernels can get wrong: beta = 0, padded leading
dimensions and an offset base, one plan at several widths, C-tile keys that
are not direct, the 32-bit offset guard, the fallback when the C-tile keys
cannot hold the matrix, unsorted rows with duplicates, exact bucket sizes,
edges of m, and argument validation.

Every test first asserts the shape (which kernels run: DeviceCSR.spmm_info()
against sblas.spmm_shape_host and the expected form), then every entry of C
against the oracle within spmm_cases.spmm_bound.  The "forms" are spmm_cases.FORMS:
row-wave, split-k, MFMA tiles with a sparse tail, C-tile fast, C-tile not fast
(B row-major with an odd row stride)."""
import numpy as np
import pytest

from spmm_cases import DUP_CASE, FORM_CASE, FORMS, case_shape, spmm_bound, spmm_case

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
# form -> (rowform, ctile, MFMA blocks?)
KERNELS = {"rowwave": (1, 0, False), "splitk": (2, 0, False), "mfma": (1, 0, True), "ctfast": (0, 1, False),
           "ctslow": (0, 1, False)}


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = spmm_case(name)
        return cache[name]
    return get


def form_ldb(form, n):
    """row-major row stride of a form: packed, except "ctslow" (odd or even, never fast at n % 16 == 0)"""
    return n + 1 if form == "ctslow" and n % 2 == 0 else n


def make_B(rng, c, n, nan_unref=True):
    """B (k x n) with NaN in every row that no entry of A references"""
    B = rng.standard_normal((c["k"], n))
    if nan_unref:
        dead = np.ones(c["k"], bool)
        dead[c["col"]] = False
        B[dead] = np.nan
    return B


def upload_B(torch, B, layout, ldb, offset=0):
    """B on the device in `layout` with leading dimension ldb, every pad entry NaN; `offset`
    doubles in front of it (a torch allocation is at least 16-byte aligned)"""
    k, n = B.shape
    if layout == 1:
        buf = np.full((k, ldb), np.nan)
        buf[:, :n] = B
    else:
        buf = np.full((n, ldb), np.nan)
        buf[:, :k] = B.T
    flat = np.concatenate([np.full(offset, np.nan), buf.ravel()])
    Bd = torch.from_numpy(flat).cuda()
    assert Bd.data_ptr() % 16 == 0
    return Bd, Bd.data_ptr() + 8 * offset


def upload_C(torch, C0, ldc):
    m, n = C0.shape
    buf = np.full((n, ldc), SENTINEL)
    buf[:, :m] = C0.T
    return torch.from_numpy(buf.ravel()).cuda()


def nan_sevenths(C0):
    C = C0.copy(order="F")
    C.ravel(order="F")[::7] = np.nan
    return C


def call_and_check(torch, sb, orc, A, c, n, n_plan, rng, *, alpha=-0.7, beta=0.8, layout=1, ldb=None, ldc=None,
                   offset=0, kernels=None, fast=None, B=None):
    """One sblas_spmm on handle A of case c (inside the case's test options): asserts the shape
    the handle took against the host function's, then C against the oracle."""
    m, k, rp, col, val = c["m"], c["k"], c["rp"], c["col"], c["val"]
    if ldb is None:
        ldb = n if layout == 1 else k
    ldc = m if ldc is None else ldc
    B = make_B(rng, c, n) if B is None else B
    C0 = rng.standard_normal((m, n))
    Cin = nan_sevenths(C0) if beta == 0.0 else C0  # beta == 0 must not read C
    Bd, b_addr = upload_B(torch, B, layout, ldb, offset)
    Cd = upload_C(torch, Cin, ldc)
    A.spmm(n, alpha, b_addr, ldb, layout, beta, Cd.data_ptr(), ldc)
    torch.cuda.synchronize()
    want_shape = sb.spmm_shape_host(k, rp, col, n_plan, ncols=n, ldb=ldb, b_layout=layout, b_addr=b_addr, beta=beta)
    T = A.spmm_info()
    assert T == want_shape
    assert (T["transposes_B"], T["kbeta"]) == (int(layout == 0), int(beta != 0.0))
    if kernels is not None:
        assert (T["rowform"], T["ctile"], T["nmfma"] > 0) == kernels
    if fast is not None:
        assert T["fast"] == fast
    out = Cd.cpu().numpy().reshape((n, ldc))
    assert np.array_equal(out[:, m:].view(np.int64), np.full((n, ldc - m), SENTINEL).view(np.int64))  # pad rows
    got = out[:, :m].T
    Cref = np.zeros((m, n)) if beta == 0.0 else C0
    want = orc.spmm(m, n, k, alpha, rp, col, val, B, beta, Cref)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= spmm_bound(rp, col, val, B, alpha, beta, Cref))
    return T


def open_case(sb, c):
    return sb.DeviceCSR.upload(0, c["k"], c["rp"], c["col"], c["val"])


# ---- 1. split-k next to MFMA blocks ------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", [1, 16, 100])
def test_splitk_beside_mfma(torch_cuda, sb, orc, cases, n, layout):
    """k_spmm_rowsplitk through rows[] (its rows follow 3 MFMA blocks), with the
    column tail n % 64 != 0; only the referenced rows of B are finite"""
    c = cases("splitk_mfma")
    A = open_case(sb, c)
    T = call_and_check(torch_cuda, sb, orc, A, c, n, n, np.random.default_rng(n + layout), layout=layout,
                       kernels=(2, 0, True))
    assert {key: T[key] for key in case_shape("splitk_mfma", c, n)} == case_shape("splitk_mfma", c, n)
    A.close()


# ---- 2. beta = 0 must not read C ---------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 100])
@pytest.mark.parametrize("form", FORMS)
def test_beta_zero_ignores_C(torch_cuda, sb, orc, cases, form, n):
    """the kBeta = false kernels: C0 holds NaN in every seventh entry, the result is finite and
    that of C0 = 0"""
    c = cases(FORM_CASE[form])
    fast = {"ctfast": int(n == 64), "ctslow": 0}.get(form, 0)
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        call_and_check(torch_cuda, sb, orc, A, c, n, n, np.random.default_rng(n), beta=0.0, ldb=form_ldb(form, n),
                       kernels=KERNELS[form], fast=fast)
        A.close()


@pytest.mark.parametrize("split", ["rows", "cols"])
@pytest.mark.parametrize("ngpu", [1, 3])
def test_csrmm_beta_zero_ignores_host_C(torch_cuda, sb, orc, cases, ngpu, split):
    """sblas_csrmm_mgpu / _colsplit skip the upload of C at beta = 0: NaN in the host C must not
    reach the result"""
    c = cases("rowwave")
    m, k, rp, col, val = c["m"], c["k"], c["rp"], c["col"], c["val"]
    n = 40
    rng = np.random.default_rng(ngpu)
    B = rng.standard_normal((k, n))
    Cf = nan_sevenths(rng.standard_normal((m, n)))
    Bf = np.asfortranarray(B)
    rp32 = rp.astype(np.int32)
    a = np.array([-0.7]); b = np.array([0.0])
    fn = sb.lib.sblas_csrmm_mgpu if split == "rows" else sb.lib.sblas_csrmm_mgpu_colsplit
    rc = fn(m, n, k, sb.ptr(a), int(rp[-1]), sb.ptr(rp32), sb.ptr(col), sb.ptr(val), sb.ptr(b), Bf.ctypes.data,
            Cf.ctypes.data, ngpu)
    assert rc == 0
    Z = np.zeros((m, n))
    want = orc.spmm(m, n, k, -0.7, rp32, col, val, B, 0.0, Z)
    assert np.all(np.isfinite(Cf))
    assert np.all(np.abs(Cf - want) <= spmm_bound(rp, col, val, B, -0.7, 0.0, Z))


# ---- 3. leading dimensions, padding and alignment ----------------------------
@pytest.mark.parametrize("bvar", ["row+1", "row+2", "col+5"])
@pytest.mark.parametrize("n", [16, 40])
@pytest.mark.parametrize("form", FORMS)
def test_leading_dimensions(torch_cuda, sb, orc, cases, form, n, bvar):
    """ldc = m + 1 and m + 3 (the pad rows of C come back bit-identical), B row-major with stride
    n + 1 / n + 2 or column-major with k + 5; every pad entry of B and every row of B that A does
    not reference is NaN"""
    c = cases(FORM_CASE[form])
    layout = 0 if bvar == "col+5" else 1
    ldb = {"row+1": n + 1, "row+2": n + 2, "col+5": c["k"] + 5}[bvar]
    fast = None
    if KERNELS[form][1]:  # C-tile: the odd stride n + 1 is never fast; n + 2 and the panel are at n = 16
        fast = int(n == 16 and bvar != "row+1")
    rng = np.random.default_rng(n)
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        for ldc in (c["m"] + 1, c["m"] + 3):
            call_and_check(torch_cuda, sb, orc, A, c, n, n, rng, layout=layout, ldb=ldb, ldc=ldc,
                           kernels=KERNELS[form], fast=fast)
        A.close()


@pytest.mark.parametrize("form", FORMS)
def test_offset_base(torch_cuda, sb, orc, cases, form):
    """B one double past a 16-byte boundary, n = 16, even stride: not fast, and right"""
    c = cases(FORM_CASE[form])
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        call_and_check(torch_cuda, sb, orc, A, c, 16, 16, np.random.default_rng(3), ldb=18, offset=1,
                       kernels=KERNELS[form], fast=0)
        if KERNELS[form][1]:  # the same call on the boundary is fast
            call_and_check(torch_cuda, sb, orc, A, c, 16, 16, np.random.default_rng(4), ldb=18, offset=2, fast=1)
        A.close()


# ---- 4. one handle at several widths -----------------------------------------
@pytest.mark.parametrize("widths", [((64, 1), (16, 0), (100, 0), (1, 1), (64, 0), (16, 1)),
                                    ((1, 1), (64, 0), (100, 1), (100, 0))],
                         ids=["built64", "built1"])
@pytest.mark.parametrize("form", ["rowwave", "ctfast"])
def test_one_plan_many_widths(torch_cuda, sb, orc, cases, form, widths):
    """the plan is built by the first call (C-tile: ns = 32 / 16-column groups of that width) and
    serves every later width; the partials and the row-major panel regrow"""
    c = cases(FORM_CASE[form])
    n_plan = widths[0][0]
    rng = np.random.default_rng(n_plan)
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        for n, layout in widths:
            T = call_and_check(torch_cuda, sb, orc, A, c, n, n_plan, rng, layout=layout, kernels=KERNELS[form])
            if form == "ctfast":
                assert T["ns"] == (8 if n_plan == 64 else 32) and T["fast"] == int(n % 16 == 0)
        A.close()


# ---- 5-7. wide matrices: B is built on the device ----------------------------
def wide_call(torch, sb, orc, A, c, n, ldb, rng, n_plan):
    """B (k x ldb, row-major) NaN-filled on the device with only the referenced rows written; the
    oracle runs on the compacted problem (referenced columns renumbered in ascending order: each
    row keeps its storage order, so sums and bound are the same)"""
    m, k, rp, col, val = c["m"], c["k"], c["rp"], c["col"], c["val"]
    used = np.unique(col)
    ccol = np.searchsorted(used, col).astype(np.int32)
    Bs = rng.standard_normal((len(used), n))
    C0 = rng.standard_normal((m, n))
    Bd = torch.full((k * ldb,), float("nan"), dtype=torch.float64, device="cuda")
    Bd.view(k, ldb)[torch.from_numpy(used.astype(np.int64)).cuda(), :n] = torch.from_numpy(Bs).cuda()
    Cd = torch.from_numpy(np.asfortranarray(C0).ravel(order="F")).cuda()
    A.spmm(n, -0.7, Bd.data_ptr(), ldb, 1, 0.8, Cd.data_ptr(), m)
    torch.cuda.synchronize()
    T = A.spmm_info()
    assert T == sb.spmm_shape_host(k, rp, col, n_plan, ncols=n, ldb=ldb, b_layout=1, b_addr=Bd.data_ptr(), beta=0.8)
    got = Cd.cpu().numpy().reshape((n, m)).T
    want = orc.spmm(m, n, len(used), -0.7, rp, ccol, val, Bs, 0.8, C0)
    assert np.all(np.abs(got - want) <= spmm_bound(rp, ccol, val, Bs, -0.7, 0.8, C0))
    return T


@pytest.mark.parametrize("n,fast", [(16, 1), (5, 0)])
def test_nondirect_keys(torch_cuda, sb, orc, cases, n, fast):
    """k > 2^21 at rbits = 11: keys hold XCD-local columns (k_spmm_ctile<false, *, false>), every
    residue of the slabs, the first, the last whole and the partial slab"""
    c = cases("nondirect")
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        T = wide_call(torch_cuda, sb, orc, A, c, n, n, np.random.default_rng(n), n)
        A.close()
    assert {key: T[key] for key in case_shape("nondirect", c, n)} == case_shape("nondirect", c, n)
    assert (T["ctile"], T["direct"], T["rbits"], T["fast"]) == (1, 0, 11, fast)


def test_offset_guard_4gib(torch_cuda, sb, orc, cases):
    """n = 16 with row stride 256 over k = 2^21 + 4133 rows: B spans 4.3 GB, beyond 32-bit byte
    offsets, so the fast kernel must not run (its offsets would wrap onto wrong rows, NaN here)"""
    c = cases("nondirect")
    assert c["k"] * 256 * 8 >= 2 ** 32
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        T = wide_call(torch_cuda, sb, orc, A, c, 16, 256, np.random.default_rng(6), 16)
        A.close()
    assert (T["ctile"], T["direct"], T["fast"]) == (1, 0, 0)


def test_unsupported_ctile_falls_back(torch_cuda, sb, orc, cases):
    """k = 2^24 + 2^14 + 1: 1,026 slabs per XCD do not fit the key at rbits = 11; the C-tile form
    asked for is refused and the row kernels serve the call"""
    c = cases("unsupported")
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        T = wide_call(torch_cuda, sb, orc, A, c, 1, 1, np.random.default_rng(7), 1)
        A.close()
    assert {key: T[key] for key in case_shape("unsupported", c, 1)} == case_shape("unsupported", c, 1)
    assert (T["ct_supported"], T["ctile"], T["rowform"]) == (0, 0, 1)


# ---- 8. unsorted columns and duplicates --------------------------------------
@pytest.mark.parametrize("n", [16, 100])
@pytest.mark.parametrize("form", FORMS)
def test_unsorted_rows_with_duplicates(torch_cuda, sb, orc, cases, form, n):
    """columns in random order, 10-30% of a row's entries repeat a column; the MFMA case holds a
    block that is dense only through its duplicates.  The oracle sums in storage order."""
    c = cases(DUP_CASE[form])
    fast = {"ctfast": int(n == 16), "ctslow": 0}.get(form, 0)
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        T = call_and_check(torch_cuda, sb, orc, A, c, n, n, np.random.default_rng(n), ldb=form_ldb(form, n),
                           kernels=KERNELS[form], fast=fast)
        A.close()
    assert {key: T[key] for key in case_shape(DUP_CASE[form], c, n)} == case_shape(DUP_CASE[form], c, n)


# ---- 9. exact C-tile bucket sizes --------------------------------------------
@pytest.mark.parametrize("n", [16, 5])
@pytest.mark.parametrize("nnz", [0, 1, 63, 64, 65, 1023, 1024, 1025, 1088])
def test_ctile_bucket_sizes(torch_cuda, sb, orc, nnz, n):
    """all entries in one bucket (columns below 2,048: slab 0 of XCD 0, its first set; one row
    block), sized around the wave iteration (64) and the workgroup stride (1,024); the other
    31 sets and 7 XCDs are empty and add exact zeros"""
    rng = np.random.default_rng(nnz)
    m, k = 300, 5000
    rows = np.sort(rng.integers(0, m, nnz))
    c = dict(m=m, k=k, rp=np.searchsorted(rows, np.arange(m + 1)).astype(np.int64),
             col=rng.integers(0, 2048, nnz).astype(np.int32), val=rng.standard_normal(nnz), opts={"spmm_ctile": 1})
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        for beta in (0.0, 0.8):
            T = call_and_check(torch_cuda, sb, orc, A, c, n, n, rng, beta=beta, kernels=(0, 1, False),
                               fast=int(n == 16))
            assert (T["wlog"], T["nrb"], T["ns"], T["R"]) == (11, 1, 32, m)
            assert nnz == 0 or c["col"].max() >> T["wlog"] == 0
        if nnz == 0:  # beta = 0: exactly zero
            Cd = torch_cuda.full((m * n,), float("nan"), dtype=torch_cuda.float64, device="cuda")
            Bd = torch_cuda.full((k * n,), float("nan"), dtype=torch_cuda.float64, device="cuda")
            A.spmm(n, 1.5, Bd.data_ptr(), n, 1, 0.0, Cd.data_ptr(), m)
            torch_cuda.cuda.synchronize()
            got = Cd.cpu().numpy()
            assert np.all(got == 0.0)
        A.close()


# ---- 10. edges of m ----------------------------------------------------------
def edge_matrix(form, m):
    rng = np.random.default_rng(m)
    k = 5000
    if form == "mfma":  # every row over the same 37 columns
        cols = np.sort(rng.choice(k, 37, replace=False))
        rows = [cols[rng.random(37) < 0.9] for _ in range(m)]
    else:
        rows = [np.sort(rng.choice(k, int(rng.integers(1, 40)), replace=False)) for _ in range(m)]
    lens = np.array([len(r) for r in rows])
    return dict(m=m, k=k, rp=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                col=np.concatenate(rows).astype(np.int32), val=rng.standard_normal(int(lens.sum())),
                opts={"ctile": {"spmm_ctile": 1}}.get(form, {}))


@pytest.mark.parametrize("m", [1, 15, 16, 17])
@pytest.mark.parametrize("form", ["row", "mfma", "ctile"])
def test_edges_of_m(torch_cuda, sb, orc, form, m):
    c = edge_matrix(form, m)
    kernels = {"row": (1, 0, False), "ctile": (0, 1, False)}.get(form)
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        for n in (40, 16):
            T = call_and_check(torch_cuda, sb, orc, A, c, n, 40, np.random.default_rng(n), kernels=kernels)
            if form == "mfma":  # whole blocks on MFMA; the lone row of m = 1 or 17 is too thin (its own union)
                assert (T["nmfma"], T["nsparse"]) == {1: (0, 1), 15: (1, 0), 16: (1, 0), 17: (1, 1)}[m]
            if form == "ctile":
                assert (T["nrb"], T["R"]) == (1, m)
        A.close()


@pytest.mark.parametrize("form", ["row", "mfma0", "ctile"])
def test_empty_tail_rows(torch_cuda, sb, orc, cases, form):
    """the last 40 rows of A are empty: their C is beta * C0 (and 0 at beta = 0)"""
    c = dict(cases("empty_tail"))
    c["opts"] = {"row": {}, "mfma0": {"spmm_mfma_fill": 0}, "ctile": {"spmm_ctile": 1}}[form]
    with sb.test_options(**c["opts"]):
        A = open_case(sb, c)
        for beta in (0.8, 0.0):
            T = call_and_check(torch_cuda, sb, orc, A, c, 40, 40, np.random.default_rng(1), beta=beta)
            if form == "row":
                assert (T["rowform"], T["nmfma"], T["ctile"]) == (1, 0, 0)
            elif form == "mfma0":  # fill 0: the blocks that hold an entry; the empty ones stay row-wave
                blocks = [(b, min(b + 16, c["m"])) for b in range(0, c["m"], 16)]
                empty = [(b0, b1) for b0, b1 in blocks if c["rp"][b1] == c["rp"][b0]]
                assert len(empty) >= 2 and T["nsparse"] == sum(b1 - b0 for b0, b1 in empty)
                assert (T["nmfma"], T["rowform"], T["ctile"]) == (len(blocks) - len(empty), 1, 0)
            else:
                assert (T["rowform"], T["nmfma"], T["ctile"]) == (0, 0, 1)
        A.close()


# ---- 11. argument validation -------------------------------------------------
def test_argument_validation(torch_cuda, sb, cases):
    """bad arguments are SBLAS_ERR_INVALID and leave C alone; n = 0 is OK and leaves C alone"""
    torch = torch_cuda
    c = cases("rowwave")
    m, k, n = c["m"], c["k"], 16
    A = open_case(sb, c)
    Bd = torch.zeros(k * (n + 8), dtype=torch.float64, device="cuda")
    Cd = torch.full((m * n,), SENTINEL, dtype=torch.float64, device="cuda")

    def call(n_, ldb, layout, ldc):
        return sb.lib.sblas_spmm(A.h, n_, 1.0, Bd.data_ptr(), ldb, layout, 0.5, Cd.data_ptr(), ldc, None)

    assert call(n, n, 1, m - 1) == 1      # ldc < m
    assert call(n, n - 1, 1, m) == 1      # row-major ldb < n
    assert call(n, k - 1, 0, m) == 1      # column-major ldb < k
    assert call(n, n, 2, m) == 1          # b_layout
    assert call(n, n, -1, m) == 1
    assert call(-1, n, 1, m) == 1         # n < 0
    assert sb.lib.sblas_spmm(None, n, 1.0, Bd.data_ptr(), n, 1, 0.5, Cd.data_ptr(), m, None) == 1
    assert call(0, n, 1, m) == 0          # n == 0
    torch.cuda.synchronize()
    assert np.array_equal(Cd.cpu().numpy().view(np.int64), np.full(m * n, SENTINEL).view(np.int64))
    assert call(n, n, 1, m) == 0          # and the handle still works
    torch.cuda.synchronize()
    assert not np.any(Cd.cpu().numpy() == SENTINEL)
    A.close()
