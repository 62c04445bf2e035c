"""sblas_csr_set_values / sblas_ctx_matrix_set_values: new values on a handle
whose pattern and analysed plans stay.

The yardstick throughout is a FRESH handle (or context) made from the same
pattern with the new values and analysed the same way under the same test
options: the refreshed handle's xsort plan buffers are byte-equal to the fresh
one's, and its y is bitwise equal for every deterministic algorithm (ROWSPLIT,
CSR5, PANEL, xsort in deterministic mode); xsort's default mode meets the
per-row bound of tests/test_spmv_gpu.py against the oracle.  The matrices are
those of tests/test_xsort_devplan_gpu.py (padding tails, blocks of 0, 1, 255,
256, 257, 512, 513 and 1024 entries, duplicates, empty rows, long rows); the
oracle's y for each matrix and value set is computed once and shared.
"""
import numpy as np
import pytest

from spmm_cases import spmm_case
from test_spmm_args_gpu import call_and_check
from test_spmv_gpu import check
from test_xsort_devplan_gpu import ALPHA, BETA, OPT_IDS, OPTS, exports, problem

pytestmark = pytest.mark.gpu

ROWSPLIT, CSR5, PANEL, XSORT = 1, 2, 4, 5
NAMES = ["ragged", "chunk_edges", "unsorted_dups", "mostly_empty", "many_groups", "no_entries", "one_dense_row",
         "last_row_full", "unit_rows"]
# (form, algo, test options): every deterministic form of tests/test_spmv_gpu.py ALGOS
FORMS = [("rowsplit", 1, {}), ("rowsplit_panel3", 1, {"rs_panel": 1, "panels": 3}), ("csr5", 2, {}),
         ("csr5_hostplan", 2, {"csr5_hostplan": 1}), ("csr5_panel2", 2, {"csr5_panel": 1, "panels": 2}),
         ("csr5_panel3", 2, {"csr5_panel": 1, "panels": 3}), ("csr5_panel8", 2, {"csr5_panel": 1, "panels": 8}),
         ("panel", 4, {}), ("panel3", 4, {"panels": 3}), ("panel8", 4, {"panels": 8}), ("auto", 0, {})]
_VALS, _WANT = {}, {}


def values(orc, name, k):
    """value set k (2, 3, ...) of a matrix; set 1 is problem()'s own val"""
    if (name, k) not in _VALS:
        val = problem(orc, name)[3]
        v = val if k == 1 else np.random.default_rng(7000 + k).standard_normal(len(val))
        if k != 1:
            v.setflags(write=False)
        _VALS[name, k] = v
    return _VALS[name, k]


def oracle(orc, name, k, beta=BETA):
    """(want, bound) of y = ALPHA*A*x + beta*y0 with value set k: once per key"""
    if (name, k, beta) not in _WANT:
        n, rp, col, _, x, y0 = problem(orc, name)[:6]
        v = values(orc, name, k)
        _WANT[name, k, beta] = (orc.csr_spmv(rp, col, v, x, ALPHA, beta, y0),
                                orc.spmv_bound(rp, col, v, x, ALPHA, beta, y0))
    return _WANT[name, k, beta]


def within(got, want_bound):
    want, bound = want_bound
    err = np.abs(got - want)
    assert np.all(err <= bound), f"max excess {np.max(err - bound)} at {np.argmax(err - bound)}"
    assert np.all(err <= 1e-3 * np.maximum(1.0, np.abs(want)))


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def run(torch, A, algo, xd, y0, beta=BETA):
    yd = dev(torch, y0)
    A.spmv(algo, ALPHA, xd.data_ptr(), beta, yd.data_ptr())
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def set_values(torch, A, v, stream=None):
    vd = dev(torch, v)
    A.set_values(vd.data_ptr(), stream)
    torch.cuda.synchronize()  # vd is read in stream order: keep it until then


def fresh(sb, orc, name, k, algo, det=False):
    n, rp, col = problem(orc, name)[:3]
    F = sb.DeviceCSR.upload(0, n, rp, col, values(orc, name, k))
    F.deterministic = det
    F.analyse(algo)
    return F


ZERO_INFO = {"calls": 0, "map_algos": 0, "map_bytes": 0, "map_build_s": 0.0, "rebuilt": False, "dropped_spmm": False}


# ---- 1, 2. the xsort layout ---------------------------------------------------
def xsort_identity(torch, sb, orc, name, opts):
    """R: uploaded with val, analysed, refreshed to v2 then v3 (the second call
    is the steady state: the map is reused).  After each call every plan
    buffer equals a fresh handle's.  Returns R's export 4 (the map)."""
    x, y0 = problem(orc, name)[4:6]
    xd = dev(torch, x)
    with sb.test_options(**opts):
        R = fresh(sb, orc, name, 1, XSORT)
        try:
            assert R.values_info() == ZERO_INFO
            with pytest.raises(sb.SblasError, match="invalid argument"):
                R.xsort_export(4)
            bytes0, info0, first = R.plan_bytes(XSORT), R.xsort_info(), None
            for calls, k in enumerate((2, 3), 1):
                set_values(torch, R, values(orc, name, k))
                F = fresh(sb, orc, name, k, XSORT)
                try:
                    for w, (a, b) in enumerate(zip(exports(R), exports(F))):
                        assert a.shape == b.shape, f"set {k}, export {w}: {a.shape} vs {b.shape}"
                        assert np.array_equal(a, b), f"set {k}, export {w} differs at byte {np.argmax(a != b)}"
                    assert R.xsort_info() == F.xsort_info() == info0
                    assert R.plan_bytes(XSORT) == F.plan_bytes(XSORT) == bytes0
                    within(run(torch, R, XSORT, xd, y0), oracle(orc, name, k))
                    R.deterministic = F.deterministic = True
                    assert np.array_equal(run(torch, R, XSORT, xd, y0), run(torch, F, XSORT, xd, y0))
                    R.deterministic = False
                    assert F.values_info() == ZERO_INFO
                finally:
                    F.close()
                vi = R.values_info()
                chunks = info0["chunks"]
                assert (vi["calls"], vi["rebuilt"], vi["dropped_spmm"]) == (calls, False, False)
                assert vi["map_bytes"] == 1024 * chunks
                assert vi["map_algos"] == ((1 << XSORT) if chunks else 0)
                if first is None:
                    first = vi
                    assert (vi["map_build_s"] > 0.0) == (chunks > 0)
                else:  # one map build: the second call found the map
                    assert vi["map_build_s"] == first["map_build_s"]
            if info0["chunks"] == 0:
                return None
            vmap = R.xsort_export(4).view(np.int32)
            # the map names every entry once; the storage is its gather
            nnz = len(values(orc, name, 1))
            assert np.array_equal(np.sort(vmap[vmap >= 0]), np.arange(nnz))
            store = R.xsort_export(0).reshape(-1, 3072)[:, 1024:].copy().view(np.float64).ravel()
            assert np.array_equal(store, np.where(vmap >= 0, values(orc, name, 3)[np.maximum(vmap, 0)], 0.0))
            return vmap
        finally:
            R.close()


@pytest.mark.parametrize("opts", OPTS, ids=OPT_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_xsort_layout_identity(torch_cuda, sb, orc, name, opts):
    xsort_identity(torch_cuda, sb, orc, name, opts)


def test_xsort_chunk_edges_single_range(torch_cuda, sb, orc):
    xsort_identity(torch_cuda, sb, orc, "chunk_edges", {"xs_cap": 1e9})


@pytest.mark.parametrize("name", ["ragged", "unsorted_dups"])
def test_xsort_host_built_layout(torch_cuda, sb, orc, name):
    """A host-built plan derives its map with the host builder: the same map
    as the device-built plan's."""
    hmap = xsort_identity(torch_cuda, sb, orc, name, {"xs_hostplan": 1})
    dmap = xsort_identity(torch_cuda, sb, orc, name, {})
    assert np.array_equal(hmap, dmap)


# ---- 3. the deterministic algorithms ------------------------------------------
@pytest.mark.parametrize("beta", [0.0, BETA])
@pytest.mark.parametrize("name", ["ragged", "mostly_empty", "no_entries", "one_dense_row"])
@pytest.mark.parametrize("form,algo,opts", FORMS, ids=[f[0] for f in FORMS])
def test_deterministic_forms(torch_cuda, sb, orc, form, algo, opts, name, beta):
    torch = torch_cuda
    x, y0 = problem(orc, name)[4:6]
    xd = dev(torch, x)
    with sb.test_options(**opts):
        R = fresh(sb, orc, name, 1, algo)
        F = fresh(sb, orc, name, 2, algo)
        try:
            set_values(torch, R, values(orc, name, 2))
            assert [R.panels(a) for a in (1, 2, 4)] == [F.panels(a) for a in (1, 2, 4)]
            got = run(torch, R, algo, xd, y0, beta)
            assert np.array_equal(got, run(torch, F, algo, xd, y0, beta))
            within(got, oracle(orc, name, 2, beta))
            assert not R.values_info()["rebuilt"]
            # the steady state: a second refresh through the resident maps
            set_values(torch, R, values(orc, name, 3))
            within(run(torch, R, algo, xd, y0, beta), oracle(orc, name, 3, beta))
        finally:
            R.close()
            F.close()


# ---- 4. several plans on one handle ---------------------------------------------
def test_several_plans_one_handle(torch_cuda, sb, orc):
    torch = torch_cuda
    name = "ragged"
    x, y0 = problem(orc, name)[4:6]
    xd = dev(torch, x)
    with sb.test_options(panels=3, csr5_panel=1):
        R = fresh(sb, orc, name, 1, ROWSPLIT, det=True)
        F = {}
        try:
            for a in (CSR5, PANEL):
                R.analyse(a)
            set_values(torch, R, values(orc, name, 2))
            vi = R.values_info()
            assert vi["map_algos"] == (1 << CSR5) | (1 << PANEL) and not vi["rebuilt"]
            R.analyse(XSORT)  # a plan analysed after a set_values: from the new values
            for a in (ROWSPLIT, CSR5, PANEL, XSORT):
                F[a] = fresh(sb, orc, name, 2, a, det=True)
                assert np.array_equal(run(torch, R, a, xd, y0), run(torch, F[a], a, xd, y0)), a
                F[a].close()
            within(run(torch, R, XSORT, xd, y0), oracle(orc, name, 2))
            set_values(torch, R, values(orc, name, 3))  # ... and refreshed by the next call
            vi = R.values_info()
            assert vi["map_algos"] == (1 << CSR5) | (1 << PANEL) | (1 << XSORT) and vi["calls"] == 2
            for a in (ROWSPLIT, CSR5, PANEL, XSORT):
                F[a] = fresh(sb, orc, name, 3, a, det=True)
                got = run(torch, R, a, xd, y0)
                assert np.array_equal(got, run(torch, F[a], a, xd, y0)), a
                within(got, oracle(orc, name, 3))
                F[a].close()
        finally:
            R.close()
            for h in F.values():
                h.close()


# ---- 5. stream order --------------------------------------------------------------
def test_stream_order(torch_cuda, sb, orc):
    """spmv, set_values, spmv on one non-default stream with no host sync in
    between: the first y is val's, the second v2's."""
    torch = torch_cuda
    name = "ragged"
    x, y0 = problem(orc, name)[4:6]
    with sb.test_options(panels=3):
        R = fresh(sb, orc, name, 1, PANEL)
        F1 = fresh(sb, orc, name, 1, PANEL)
        F2 = fresh(sb, orc, name, 2, PANEL)
        try:
            xd = dev(torch, x)
            set_values(torch, R, values(orc, name, 1))  # the map build (which waits) out of the way
            ya, yb, vd = dev(torch, y0), dev(torch, y0), dev(torch, values(orc, name, 2))
            torch.cuda.synchronize()
            st = torch.cuda.Stream()
            s = st.cuda_stream
            R.spmv(PANEL, ALPHA, xd.data_ptr(), BETA, ya.data_ptr(), s)
            R.set_values(vd.data_ptr(), s)
            R.spmv(PANEL, ALPHA, xd.data_ptr(), BETA, yb.data_ptr(), s)
            st.synchronize()
            assert np.array_equal(ya.cpu().numpy(), run(torch, F1, PANEL, xd, y0))
            assert np.array_equal(yb.cpu().numpy(), run(torch, F2, PANEL, xd, y0))
            within(yb.cpu().numpy(), oracle(orc, name, 2))
        finally:
            for h in (R, F1, F2):
                h.close()


# ---- 6. no room for a map -----------------------------------------------------------
@pytest.mark.parametrize("algo,opts", [(XSORT, {}), (PANEL, {"panels": 3}), (ROWSPLIT, {"rs_panel": 1, "panels": 3}),
                                       (CSR5, {"csr5_panel": 1, "panels": 3})],
                         ids=["xsort", "panel3", "rowsplit_panel3", "csr5_panel3"])
def test_map_allocation_failure_rebuilds(torch_cuda, sb, orc, algo, opts):
    torch = torch_cuda
    name = "ragged"
    x, y0 = problem(orc, name)[4:6]
    xd = dev(torch, x)
    with sb.test_options(**opts):
        R = fresh(sb, orc, name, 1, algo, det=True)
        F = fresh(sb, orc, name, 2, algo, det=True)
        try:
            panels = R.panels(algo)
            with sb.test_options(sv_map_nomem=1):
                set_values(torch, R, values(orc, name, 2))
            vi = R.values_info()
            assert vi["rebuilt"] and vi["map_bytes"] == 0 and vi["map_algos"] == 0 and vi["calls"] == 1
            assert R.panels(algo) == panels == F.panels(algo)
            got = run(torch, R, algo, xd, y0)
            assert np.array_equal(got, run(torch, F, algo, xd, y0))
            within(got, oracle(orc, name, 2))
            if algo == XSORT:
                for a, b in zip(exports(R), exports(F)):
                    assert np.array_equal(a, b)
        finally:
            R.close()
            F.close()


# ---- 7. SpMM and transpose ------------------------------------------------------------
@pytest.mark.parametrize("case", ["ct", "mfma"])
def test_spmm_plan_is_dropped_and_rebuilt(torch_cuda, sb, orc, case):
    torch = torch_cuda
    c = spmm_case(case)
    rng = np.random.default_rng(17)
    v2 = rng.standard_normal(len(c["val"]))
    with sb.test_options(**c["opts"]):
        A = sb.DeviceCSR.upload(0, c["k"], c["rp"], c["col"], c["val"])
        try:
            T = call_and_check(torch, sb, orc, A, c, 16, 16, rng)
            assert (T["ctile"], T["nmfma"] > 0) == (int(case == "ct"), case == "mfma")
            set_values(torch, A, v2)
            assert A.values_info()["dropped_spmm"]
            with pytest.raises(sb.SblasError, match="invalid argument"):
                A.spmm_info()
            assert call_and_check(torch, sb, orc, A, dict(c, val=v2), 16, 16, rng) == T
            set_values(torch, A, c["val"])
            call_and_check(torch, sb, orc, A, c, 32, 32, rng)  # tuned to that call's width
        finally:
            A.close()


def test_transpose_reads_new_values(torch_cuda, sb, orc):
    torch = torch_cuda
    name = "unsorted_dups"
    n, rp, col = problem(orc, name)[:3]
    m, nnz = len(rp) - 1, int(rp[-1])
    v2 = values(orc, name, 2)
    A = fresh(sb, orc, name, 1, ROWSPLIT)
    try:
        set_values(torch, A, v2)
        cp = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        ri = torch.zeros(nnz, dtype=torch.int32, device="cuda")
        cv = torch.zeros(nnz, dtype=torch.float64, device="cuda")
        A.transpose(cp.data_ptr(), ri.data_ptr(), cv.data_ptr())
        torch.cuda.synchronize()
        wcp, wri, wcv = orc.transpose(m, n, rp, col, v2)
        wcp1, wri1, _ = orc.transpose(m, n, rp, col, values(orc, name, 1))
        assert np.array_equal(wcp, wcp1) and np.array_equal(wri, wri1)  # indices do not depend on values
        assert np.array_equal(cp.cpu().numpy(), wcp)
        assert np.array_equal(ri.cpu().numpy(), wri)
        assert np.array_equal(cv.cpu().numpy().view(np.int64), wcv.view(np.int64))
    finally:
        A.close()


# ---- 8. a slice handle ----------------------------------------------------------------
@pytest.mark.parametrize("algo,opts", [(ROWSPLIT, {}), (CSR5, {"csr5_panel": 1, "panels": 3}), (PANEL, {"panels": 3}),
                                       (XSORT, {})], ids=["rowsplit", "csr5_panel3", "panel3", "xsort"])
def test_slice_handle(torch_cuda, sb, orc, algo, opts):
    """upload_slice with partial first and last rows (a slice of spMV_mgpu_v1's
    nnz partition): set_values takes the slice's elements idx_begin..idx_end."""
    torch = torch_cuda
    name = "ragged"
    n, rp, col, val, x = problem(orc, name)[:5]
    nnz = int(rp[-1])
    i0, i1 = nnz // 3 + 5, 2 * nnz // 3 + 11
    r0 = int(np.searchsorted(rp, i0, side="right")) - 1
    r1 = int(np.searchsorted(rp, i1 - 1, side="right"))
    assert rp[r0] < i0 < rp[r0 + 1] and rp[r1 - 1] < i1 < rp[r1]  # partial rows at both ends
    lrp = np.clip(rp[r0:r1 + 1], i0, i1) - i0
    v2 = values(orc, name, 2)
    y0 = np.random.default_rng(5).standard_normal(r1 - r0)
    xd = dev(torch, x)
    with sb.test_options(**opts):
        R = sb.DeviceCSR.upload_slice(0, n, rp, col, val, r0, r1, i0, i1)
        F = sb.DeviceCSR.upload_slice(0, n, rp, col, v2, r0, r1, i0, i1)
        try:
            R.deterministic = F.deterministic = True
            R.analyse(algo)
            F.analyse(algo)
            assert R.info() == (r1 - r0, n, i1 - i0)
            set_values(torch, R, v2[i0:i1])
            got = run(torch, R, algo, xd, y0)
            assert np.array_equal(got, run(torch, F, algo, xd, y0))
            check(orc, lrp, col[i0:i1], v2[i0:i1], x, ALPHA, BETA, y0, got)
        finally:
            R.close()
            F.close()


# ---- 9. the context ---------------------------------------------------------------------
CTX_ALGOS = [(CSR5, {"csr5_panel": 1, "panels": 3}), (PANEL, {"panels": 3}), (XSORT, {}), (0, {})]
CTX_LAYOUTS = [(0, 0, 1), (0, 0, 2), (1, 0, 1), (1, 1, 1), (2, 0, 1), (2, 1, 1)]  # partition, exchange, parts


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("algo,opts", CTX_ALGOS, ids=["csr5_panel3", "panel3", "xsort", "auto"])
@pytest.mark.parametrize("partition,exchange,parts", CTX_LAYOUTS,
                         ids=["cyclic", "cyclic_parts2", "nnz_gather", "nnz_reduce", "cost_gather", "cost_reduce"])
def test_ctx_set_values(torch_cuda, sb, orc, monkeypatch, g, algo, opts, partition, exchange, parts):
    monkeypatch.setenv("SBLAS_CTX_LOOPBACK", "1")
    name = "ragged"
    n, rp, col, val, x, y0 = problem(orc, name)[:6]
    m = len(rp) - 1
    v2 = values(orc, name, 2)

    def load(ctx, v):
        if parts > 1:
            ctx.upload_parts(m, n, rp, col, v, algo, parts)
            assert ctx.parts() == parts
        else:
            ctx.upload(m, n, rp, col, v, algo, partition, exchange)

    def step(ctx):
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.spmv(ALPHA, BETA)
        return [ctx.get_y(d) for d in range(g)]

    with sb.test_options(**opts):
        R, F = sb.DeviceCtx(g), sb.DeviceCtx(g)
        try:
            with pytest.raises(sb.SblasError, match="invalid argument"):
                R.set_values(v2)  # nothing loaded
            load(R, val)
            load(F, v2)
            for d, y in enumerate(step(R)):
                within(y, oracle(orc, name, 1))
            R.set_values(v2)
            got, want = step(R), step(F)
            for d in range(g):
                within(got[d], oracle(orc, name, 2))
                if algo in (CSR5, PANEL):  # deterministic: the fresh context's y, bit for bit
                    assert np.array_equal(got[d], want[d]), d
            R.set_values(values(orc, name, 3))  # through the resident maps
            for y in step(R):
                within(y, oracle(orc, name, 3))
        finally:
            R.close()
            F.close()


# ---- 10. arguments ----------------------------------------------------------------------
def test_arguments(torch_cuda, sb, orc):
    torch = torch_cuda
    A = fresh(sb, orc, "one_dense_row", 1, ROWSPLIT)
    E = fresh(sb, orc, "no_entries", 1, ROWSPLIT)
    try:
        assert A.values_info() == ZERO_INFO
        assert sb.lib.sblas_csr_set_values(A.h, None, None) == 1  # SBLAS_ERR_INVALID
        assert sb.lib.sblas_csr_set_values(None, None, None) == 1
        assert sb.lib.sblas_csr_values_info(None, None) == 1
        assert A.values_info()["calls"] == 0
        E.set_values(None)  # nnz == 0
        assert E.values_info()["calls"] == 1
        torch.cuda.synchronize()
    finally:
        A.close()
        E.close()
