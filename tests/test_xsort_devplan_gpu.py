"""The xsort layout built on the device is the host-built layout, byte for byte.

Every case builds the plan twice on fresh handles -- under the test option
"xs_hostplan" (the host inspector) and by default (the device inspector) --
and compares all four plan buffers (sblas_csr_xsort_export), the plan's shape
and its device bytes; the device-built handle's y meets the per-row bound of
tests/test_spmv_gpu.py, and in deterministic mode both handles give the same y
bit for bit.

The planner cuts even a small matrix into many ranges to fill the grid (64
all-wide ranges by default), so the two cases that are about the blocks of ONE
range -- big blocks, chunk edges -- also run with a huge "xs_cap", which
leaves a single range, besides the four planner settings every matrix is
crossed with.

The chunk-edges matrix: its per-group entry counts are exactly 0, 1, 255, 256,
257, 512, 513 and 1024 (2818 entries over 771 rows, so the rows hold the same
columns up to one extra in the leading rows of a group: 771 equal rows cannot
give a count of 1).  As one range its eight blocks have exactly those sizes
(14 chunks).
"""
import numpy as np
import pytest

from test_spmv_gpu import random_csr

pytestmark = pytest.mark.gpu

XSORT = 5
OPTS = [{}, {"xs_allwide": 0}, {"xs_allwide": 0, "xs_cap": 50}, {"xs_solo": 1, "xs_cap": 50}]
OPT_IDS = ["default", "narrow", "narrow_cap50", "solo_cap50"]
EDGE_COUNTS = (0, 1, 255, 256, 257, 512, 513, 1024)


def _strata(rng, m, n, k):
    """k distinct sorted random columns per row: one from each of k strata."""
    w = n // k
    return (np.arange(k)[None, :] * w + rng.integers(0, w, size=(m, k))).astype(np.int32).ravel()


def _ragged(rng):
    m, n = 3000, 40000
    return (n,) + random_csr(rng, m, n, 60, long_rows=[(5, 2049), (17, 8192), (900, 30000)])


def _chunk_edges(rng):
    n, m = 4096, 771
    wg = (n + 7) // 8
    rows, cols = [], []
    for g, c in enumerate(EDGE_COUNTS):
        t = np.arange(c)
        rows.append(t % m)
        cols.append(g * wg + t // m)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return n, rp, cols[order].astype(np.int32), rng.standard_normal(len(order))


def _big_blocks(rng):
    m = n = 8192
    rp = np.arange(m + 1, dtype=np.int64) * 200
    return n, rp, _strata(rng, m, n, 200), rng.standard_normal(m * 200)


def _many_groups(rng):
    m, n = 2000, 2_200_000
    rp = np.arange(m + 1, dtype=np.int64) * 40
    return n, rp, _strata(rng, m, n, 40), rng.standard_normal(m * 40)


def _unsorted_dups(rng):
    m, n = 500, 3000
    lens = rng.integers(0, 60, size=m)
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    col = rng.integers(0, n, size=int(rp[-1])).astype(np.int32)  # draw order, with replacement
    assert any(len(np.unique(col[rp[r]:rp[r + 1]])) < lens[r] for r in range(m))
    return n, rp, col, rng.standard_normal(int(rp[-1]))


def _mostly_empty(rng):
    m, n = 60000, 70000
    return (n,) + random_csr(rng, m, n, 40, long_rows=[(3, 3000), (31000, 12000)], empty_frac=0.6)


def _no_entries(rng):
    return 50, np.zeros(101, np.int64), np.zeros(0, np.int32), np.zeros(0)


def _one_dense_row(rng):
    n = 1000
    return n, np.array([0, n], np.int64), np.arange(n, dtype=np.int32), rng.standard_normal(n)


def _last_row_full(rng):
    m, n = 5000, 1000
    rp = np.zeros(m + 1, np.int64)
    rp[-1] = n
    return n, rp, np.arange(n, dtype=np.int32), rng.standard_normal(n)


def _unit_rows(rng):
    m = n = 4099
    return n, np.arange(m + 1, dtype=np.int64), rng.integers(0, n, size=m).astype(np.int32), \
        rng.standard_normal(m)


MATRICES = {"ragged": _ragged, "chunk_edges": _chunk_edges, "big_blocks": _big_blocks,
            "many_groups": _many_groups, "unsorted_dups": _unsorted_dups, "mostly_empty": _mostly_empty,
            "no_entries": _no_entries, "one_dense_row": _one_dense_row, "last_row_full": _last_row_full,
            "unit_rows": _unit_rows}
_CACHE = {}
ALPHA, BETA = 1.25, 0.75


def problem(orc, name):
    """The matrix, x, y0 and the oracle's y and per-row bound: computed once
    per matrix, shared by its cases, never modified."""
    if name not in _CACHE:
        rng = np.random.default_rng(2024)
        if name == "synth320k":
            n = 320000
            rp, col, val = orc.gen_synth(n)
        else:
            n, rp, col, val = MATRICES[name](rng)
        m = len(rp) - 1
        x = rng.standard_normal(n)
        y0 = rng.standard_normal(m)
        want = orc.csr_spmv(rp, col, val, x, ALPHA, BETA, y0)
        bound = orc.spmv_bound(rp, col, val, x, ALPHA, BETA, y0)
        for a in (rp, col, val, x, y0, want, bound):
            a.setflags(write=False)
        _CACHE[name] = (n, rp, col, val, x, y0, want, bound)
    return _CACHE[name]


def exports(A):
    return [A.xsort_export(w) for w in range(4)]


def spmv(torch, A, xd, y0):
    yd = torch.from_numpy(np.array(y0)).cuda()
    A.spmv(XSORT, ALPHA, xd.data_ptr(), BETA, yd.data_ptr())
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def compare_builds(torch, sb, orc, name, opts, host_opts=None):
    """Steps 1-7 of the comparison; returns the device-built plan's shape."""
    n, rp, col, val, x, y0, want, bound = problem(orc, name)
    with sb.test_options(**dict(host_opts or {"xs_hostplan": 1}, **opts)):
        H = sb.DeviceCSR.upload(0, n, rp, col, val)
        H.analyse(XSORT)
    with sb.test_options(**opts):
        D = sb.DeviceCSR.upload(0, n, rp, col, val)
        D.analyse(XSORT)
    try:
        assert H.xsort_build_info()[0] == 0
        assert D.xsort_build_info()[0] == 1
        eh, ed = exports(H), exports(D)
        info = D.xsort_info()
        assert len(ed[0]) == info["chunks"] * 3072
        for w, (a, b) in enumerate(zip(eh, ed)):
            assert a.shape == b.shape, f"export {w}: {a.shape} vs {b.shape}"
            assert np.array_equal(a, b), f"export {w} differs at byte {np.argmax(a != b)}"
        assert H.xsort_info() == info
        assert H.plan_bytes(XSORT) == D.plan_bytes(XSORT) > 0
        xd = torch.from_numpy(np.array(x)).cuda()
        got = spmv(torch, D, xd, y0)
        err = np.abs(got - want)  # the `check` of tests/test_spmv_gpu.py against the shared reference
        assert np.all(err <= bound), f"max excess {np.max(err - bound)} at {np.argmax(err - bound)}"
        assert np.all(err <= 1e-3 * np.maximum(1.0, np.abs(want)))
        H.deterministic = True
        D.deterministic = True
        assert np.array_equal(spmv(torch, H, xd, y0), spmv(torch, D, xd, y0))
        return info
    finally:
        H.close()
        D.close()


@pytest.mark.parametrize("opts", OPTS, ids=OPT_IDS)
@pytest.mark.parametrize("name", list(MATRICES))
def test_device_layout_is_host_layout(torch_cuda, sb, orc, name, opts):
    info = compare_builds(torch_cuda, sb, orc, name, opts)
    if name == "mostly_empty" and not opts:
        assert info["solo"] == 1


@pytest.mark.parametrize("opts", [{"xs_cap": 1e9}, {"xs_allwide": 0, "xs_cap": 1e9}], ids=["wide", "narrow"])
def test_chunk_edges_single_range(torch_cuda, sb, orc, opts):
    """One range: its blocks hold exactly 0, 1, 255, 256, 257, 512, 513 and
    1024 entries (an empty block, padding tails, blocks of whole chunks)."""
    info = compare_builds(torch_cuda, sb, orc, "chunk_edges", opts)
    assert info["ranges"] == 1
    assert info["chunks"] == sum((c + 255) // 256 for c in EDGE_COUNTS) == 14


def test_big_blocks_single_range(torch_cuda, sb, orc):
    """One all-wide range: eight blocks of ~205K entries each, far more than
    one workgroup's LDS holds."""
    info = compare_builds(torch_cuda, sb, orc, "big_blocks", {"xs_cap": 1e9})
    assert (info["ranges"], info["wide"]) == (1, 1)
    # 1,638,400 entries in 8 blocks, each with at most one partly filled chunk
    assert 6400 <= info["chunks"] <= 6400 + 8


def test_default_planner_at_size(torch_cuda, sb, orc):
    """~6.4M entries, just above the all-wide limit: the production mix of
    narrow and wide ranges with real block sizes."""
    info = compare_builds(torch_cuda, sb, orc, "synth320k", {})
    assert 0 < info["wide"] < info["ranges"]


def test_from_device_handle_never_copies_entries_back(torch_cuda, sb, orc):
    torch = torch_cuda
    n, rp, col, val = problem(orc, "ragged")[:4]
    m, nnz = len(rp) - 1, int(rp[-1])
    drp = torch.from_numpy(rp.astype(np.int32)).cuda()
    dcol = torch.from_numpy(np.array(col)).cuda()
    dval = torch.from_numpy(np.array(val)).cuda()
    torch.cuda.synchronize()
    A = sb.DeviceCSR.from_device(0, m, n, nnz, drp.data_ptr(), dcol.data_ptr(), dval.data_ptr())
    try:
        A.analyse(XSORT)
        bi = A.xsort_build_info()
        assert bi.device_built == 1
        blocks = A.xsort_info()["ranges"] * 8  # n = 40000: G = 8 column groups
        # the block offsets (and the handle's rowptr copy); allowance: one more
        # 8-byte word, the count pass's bad-entry flag travelling behind blk[]
        allowance = 8
        assert 0 < bi.d2h_bytes <= 8 * (blocks + 1) + 4 * (m + 1) + allowance
        assert bi.d2h_bytes * 100 < 12 * nnz
        assert bi.scratch_bytes >= 24 * nnz
    finally:
        A.close()


@pytest.mark.parametrize("hostplan", [1, 0], ids=["host", "device"])
def test_bad_column_is_refused(torch_cuda, sb, orc, hostplan):
    """A column equal to n: both builds refuse the plan (the device build only
    counts such an entry, its column never becomes an address); the handle
    still runs the row split.  x carries one spare element, which that entry
    reads there."""
    torch = torch_cuda
    n, rp, col, val = problem(orc, "ragged")[:4]
    col = np.array(col)
    col[int(rp[901]) - 1] = n  # the last entry of the 30000-entry row
    m = len(rp) - 1
    rng = np.random.default_rng(5)
    x = np.append(rng.standard_normal(n), 0.0)
    y0 = rng.standard_normal(m)
    A = sb.DeviceCSR.upload(0, n, rp, col, val)
    try:
        with sb.test_options(xs_hostplan=hostplan):
            with pytest.raises(sb.SblasError, match="invalid argument.*column index out of"):
                A.analyse(XSORT)
        assert A.xsort_info()["ready"] == 0
        xd = torch.from_numpy(x).cuda()
        yd = torch.from_numpy(y0.copy()).cuda()
        A.spmv(1, ALPHA, xd.data_ptr(), BETA, yd.data_ptr())
        torch.cuda.synchronize()
        want = orc.csr_spmv(rp, col, val, x, ALPHA, BETA, y0)
        bound = orc.spmv_bound(rp, col, val, x, ALPHA, BETA, y0)
        assert np.all(np.abs(yd.cpu().numpy() - want) <= bound)
    finally:
        A.close()


def test_scratch_failure_falls_back(torch_cuda, sb, orc):
    """Test option "xs_devplan_nomem": the device build's scratch cannot be
    allocated, so the host build runs -- and gives the same layout as the
    device build."""
    compare_builds(torch_cuda, sb, orc, "ragged", {}, host_opts={"xs_devplan_nomem": 1})
