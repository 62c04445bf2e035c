"""Which kernel each triangular solve runs: every case first asserts the shape
of the launch (DeviceTRSV.info / TrsvMgpu.shape against sblas.trsv_shape_host,
which tests/test_trsv_shape_cpu.py pins to literal values, and the pull-kernel
instance as literals here), then the exact solution.  Integer systems: exact
equality throughout."""
import numpy as np
import pytest

from trsv_cases import chain_system, csc_matmat, from_deps, kat, three_run_system

pytestmark = pytest.mark.gpu

# rhs -> the pull instance (rp, v): natural order, level order
INSTANCE = {1: ((1, 1), (1, 1)), 2: ((1, 2), (2, 1)), 3: ((2, 2), (4, 1)), 5: ((4, 2), (8, 1)), 8: ((4, 2), (8, 1)),
            16: ((4, 4), (8, 2)), 17: ((8, 4), (16, 2)), 32: ((8, 4), (16, 2)), 64: ((8, 8), (16, 4)),
            100: ((8, 8), (16, 4))}


@pytest.fixture(scope="module")
def ncu(torch_cuda):
    return torch_cuda.cuda.get_device_properties(0).multi_processor_count


def rhs_system(system, rhs, seed=0):
    """(cp, ri, cv, B, X) with rhs integer right-hand sides (rhs 1: the system's own b, x)"""
    cp, ri, cv, b, xref = system
    if rhs == 1:
        return cp, ri, cv, b, xref
    X = np.random.default_rng(rhs + seed).integers(1, 11, (len(cp) - 1, rhs)).astype(np.float64)
    return cp, ri, cv, csc_matmat(cp, ri, cv, X), X


def solve_single(torch, sb, ncu, system, sub, rhs, algos):
    """the handle's solves: shape, then x == X, for each algo (4: as pick() resolves it)"""
    cp, ri, cv, B, X = system
    n = len(cp) - 1
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (cp, ri, cv, B)]
    T = sb.DeviceTRSV(0, n, len(ri), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), sub)
    try:
        with pytest.raises(RuntimeError):
            T.info()  # nothing solved yet
        for algo in algos:
            xd = torch.zeros(X.shape, dtype=torch.float64, device="cuda")
            if rhs == 1:
                T.solve(algo, d[3].data_ptr(), xd.data_ptr())
            else:
                T.solve_rhs_opt(algo, 3, rhs, d[3].data_ptr(), xd.data_ptr())
            torch.cuda.synchronize()
            real = T.pick() if algo == 4 else algo
            info = T.info()
            want = sb.trsv_shape_host(real, 0, rhs, False, 1, 1, ncu)
            assert {k: info[k] for k in sb.TRSV_SHAPE_KEYS} == want
            if real in (1, 3):
                assert (info["rp"], info["v"], info["sys"]) == INSTANCE[rhs][real == 3] + (0,)
            assert np.array_equal(xd.cpu().numpy(), X)
    finally:
        T.close()


def solve_blocks(sb, ncu, system, sub, rhs, blocks=3):
    """the persistent multi-device handle, two runs: block 0's shape, then x == X"""
    cp, ri, cv, B, X = system
    n = len(cp) - 1
    H = sb.TrsvMgpu(cp, ri, cv, n, blocks, substitution=sub, rhs=rhs)
    try:
        with pytest.raises(RuntimeError):
            H.shape()
        devs = [dev for dev, _ in H.info()]
        for _ in range(2):
            x, _ms = H.run(B)
            S = H.shape()
            assert S == sb.trsv_shape_host(1, 0, rhs, True, blocks, devs.count(devs[0]), ncu)
            assert (S["rp"], S["v"], S["sys"], S["threads"]) == INSTANCE[rhs][0] + (1, 256)
            assert np.array_equal(x, X)
    finally:
        H.close()


@pytest.mark.parametrize("name", ["ash85", "qh768"])
@pytest.mark.parametrize("sub", ["fwd", "bwd"])
@pytest.mark.parametrize("rhs", [2, 3, 8, 16, 17, 32, 64, 100])
def test_every_sptrsm_instance(torch_cuda, sb, ncu, name, sub, rhs):
    """Natural order, level order and three blocks over these rhs are all 18
    SpTRSM instances; n = 85 is no multiple of any 64 / rp, rhs 3, 17 and 100
    leave partial passes and lanes, rhs 100 runs two passes."""
    system = rhs_system(kat(name, sub), rhs)
    s = 0 if sub == "fwd" else 1
    solve_single(torch_cuda, sb, ncu, system, s, rhs, (1, 3))
    solve_blocks(sb, ncu, system, s, rhs)


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("rhs", [1, 5])
def test_chain_across_tickets(torch_cuda, sb, ncu, sub, rhs):
    """A bidiagonal chain of 130 rows: two full tickets plus two rows, every
    row waiting for the previous one -- the longest chain inside a wave, and
    across every ticket boundary."""
    system = rhs_system(chain_system(130, sub), rhs)
    solve_single(torch_cuda, sb, ncu, system, sub, rhs, (1, 3, 4))
    solve_blocks(sb, ncu, system, sub, rhs)
    x, _ = sb.trsv_mgpu_solve(system[0], system[1], system[2], 130, system[3], 3, sub, rhs)
    assert np.array_equal(x, system[4])


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("rhs", [1, 5])
def test_one_row(torch_cuda, sb, ncu, sub, rhs):
    """n = 1: the diagonal alone"""
    cp, ri, cv, b, xref = from_deps(1, [[]], sub)
    system = rhs_system((cp, ri, 2.0 * cv, 2.0 * b, xref), rhs)
    solve_single(torch_cuda, sb, ncu, system, sub, rhs, (1, 3, 4))
    solve_blocks(sb, ncu, system, sub, rhs)
    x, _ = sb.trsv_mgpu_solve(system[0], system[1], system[2], 1, system[3], 3, sub, rhs)
    assert np.array_equal(np.reshape(x, np.shape(system[4])), system[4])


def test_levelset_wide_narrow_wide(torch_cuda, sb, ncu):
    """Levels of 2,049 / 1 / 2,049 rows: the level-set executor runs a wide, a
    narrow and a wide run, so the grid-barrier words are reset between two
    wide runs; two solves on the handle, bit-identical to algo 1."""
    torch = torch_cuda
    cp, ri, cv, b, xref = three_run_system()
    n = len(cp) - 1
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (cp, ri, cv, b)]
    T = sb.DeviceTRSV(0, n, len(ri), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0)
    try:
        xd = torch.zeros(n, dtype=torch.float64, device="cuda")
        T.solve(1, d[3].data_ptr(), xd.data_ptr())
        torch.cuda.synchronize()
        pull = xd.cpu().numpy()
        assert T.info()["executor"] == 1 and (T.info()["narrow_runs"], T.info()["wide_runs"]) == (0, 0)
        for _ in range(2):
            xd.zero_()
            T.solve(2, d[3].data_ptr(), xd.data_ptr())
            torch.cuda.synchronize()
            info = T.info()
            assert {k: info[k] for k in sb.TRSV_SHAPE_KEYS} == sb.trsv_shape_host(2, 0, 1, False, 1, 1, ncu)
            assert (info["narrow_runs"], info["wide_runs"]) == (1, 2)
            x = xd.cpu().numpy()
            assert np.array_equal(x, pull) and np.array_equal(x, xref)
        assert T.levels() == 3
    finally:
        T.close()
