"""The triangular solve's shape on the CPU (sblas.trsv_shape_host,
sblas.trsv_levels_host: no GPU): every value a solve fixes before its launch,
as literal expected values on a 256-CU device, both sides of every threshold,
the set of pull-kernel instances that can be asked for, and the level-set
executor's narrow / wide schedule."""
import pytest

from trsv_cases import NCU, chain_system, kat, one_level_then_row, schedule_system, three_run_system

RHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 100]

# rhs -> (c, rp, v, passes, rows_per_claim)
NATURAL = {1: (1, 1, 1, 1, 64), 2: (2, 1, 2, 1, 64), 3: (4, 2, 2, 1, 32), 4: (4, 2, 2, 1, 32),
           5: (8, 4, 2, 1, 16), 8: (8, 4, 2, 1, 16), 9: (16, 4, 4, 1, 16), 16: (16, 4, 4, 1, 16),
           17: (32, 8, 4, 1, 8), 32: (32, 8, 4, 1, 8), 33: (64, 8, 8, 1, 8), 64: (64, 8, 8, 1, 8),
           65: (64, 8, 8, 2, 8), 100: (64, 8, 8, 2, 8)}
LEVEL = {1: (1, 1, 1, 1, 64), 2: (2, 2, 1, 1, 32), 3: (4, 4, 1, 1, 16), 4: (4, 4, 1, 1, 16),
         5: (8, 8, 1, 1, 8), 8: (8, 8, 1, 1, 8), 9: (16, 8, 2, 1, 8), 16: (16, 8, 2, 1, 8),
         17: (32, 16, 2, 1, 4), 32: (32, 16, 2, 1, 4), 33: (64, 16, 4, 1, 4), 64: (64, 16, 4, 1, 4),
         65: (64, 16, 4, 2, 4), 100: (64, 16, 4, 2, 4)}
# natural-order SpTRSM on one handle: workgroups per CU
MULT = {2: 1, 3: 1, 4: 1, 5: 1, 8: 1, 9: 1, 15: 1, 16: 2, 17: 2, 32: 2, 33: 4, 64: 4, 65: 4, 100: 4}

TRIPLES = ({(rp, v, 0) for rp, v in [(1, 2), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8)]} |
           {(rp, v, 1) for rp, v in [(1, 2), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8)]} |
           {(rp, v, 0) for rp, v in [(2, 1), (4, 1), (8, 1), (8, 2), (16, 2), (16, 4)]})


def pull(order, c, rp, v, passes, rpc, sys, threads, grid, slp):
    return dict(executor=1, level_order=order, c=c, rp=rp, v=v, passes=passes, rows_per_claim=rpc, sys=sys,
                threads=threads, grid=grid, slp=slp)


@pytest.mark.parametrize("rhs", RHS)
def test_single_natural(sb, rhs):
    threads = 128 if rhs == 1 else 256
    grid = NCU * (1 if rhs == 1 else MULT[rhs])
    assert sb.trsv_shape_host(1, 0, rhs, False, 1, 1, NCU) == pull(0, *NATURAL[rhs], 0, threads, grid, 1)


@pytest.mark.parametrize("rhs", RHS)
def test_single_level_order(sb, rhs):
    threads = 64 if rhs == 1 else 256
    assert sb.trsv_shape_host(3, 0, rhs, False, 1, 1, NCU) == pull(1, *LEVEL[rhs], 0, threads, NCU, -6)


@pytest.mark.parametrize("rhs", RHS)
def test_mgpu_one_block(sb, rhs):
    """256 threads and, at rhs 1 alone, system scope even without peers; no grid multiplier"""
    assert sb.trsv_shape_host(1, 0, rhs, True, 1, 1, NCU) == pull(0, *NATURAL[rhs], int(rhs == 1), 256, NCU, 1)


@pytest.mark.parametrize("rhs", RHS)
def test_mgpu_three_blocks(sb, rhs):
    assert sb.trsv_shape_host(1, 0, rhs, True, 3, 3, NCU) == pull(0, *NATURAL[rhs], 1, 256, 85, 1)
    assert sb.trsv_shape_host(1, 0, rhs, True, 3, 1, NCU) == pull(0, *NATURAL[rhs], 1, 256, NCU, 1)


def test_mgpu_scope(sb):
    """system scope: the rhs 1 kernel always, the SpTRSM from two blocks on"""
    for rhs in (1, 5):
        sys = [sb.trsv_shape_host(1, 0, rhs, True, blocks, 1, NCU)["sys"] for blocks in (1, 2, 3)]
        assert sys == [int(rhs == 1), 1, 1]


@pytest.mark.parametrize("rhs", sorted(MULT))
def test_grid_multiplier(sb, rhs):
    """x 1 below rhs 16, x 2 up to 32, x 4 above: natural order on one handle only"""
    assert sb.trsv_shape_host(1, 0, rhs, False, 1, 1, NCU)["grid"] == NCU * MULT[rhs]
    assert sb.trsv_shape_host(3, 0, rhs, False, 1, 1, NCU)["grid"] == NCU
    assert sb.trsv_shape_host(1, 0, rhs, True, 1, 1, NCU)["grid"] == NCU


@pytest.mark.parametrize("k,grid", [(1, 256), (2, 128), (3, 85), (4, 64), (7, 36), (256, 1), (257, 1), (1000, 1)])
def test_blocks_sharing_a_device(sb, k, grid):
    for rhs in (1, 5):
        assert sb.trsv_shape_host(1, 0, rhs, True, 1000, k, NCU)["grid"] == grid


@pytest.mark.parametrize("opt,rhs", [(0, 1), (1, 1), (2, 1), (3, 1), (1, 17), (2, 17), (3, 17), (3, 100)])
def test_push(sb, opt, rhs):
    assert sb.trsv_shape_host(0, opt, rhs, False, 1, 1, NCU) == dict(
        executor=0, level_order=0, c=0, rp=0, v=0, passes=0, rows_per_claim=1, sys=0, threads=256, grid=NCU, slp=0)


@pytest.mark.parametrize("ncu,grid", [(256, 256), (1024, 1024), (1025, 1024), (1, 1)])
def test_levelset(sb, ncu, grid):
    assert sb.trsv_shape_host(2, 0, 1, False, 1, 1, ncu) == dict(
        executor=2, level_order=1, c=0, rp=0, v=0, passes=0, rows_per_claim=0, sys=0, threads=1024, grid=grid, slp=0)


def test_reachable_instances(sb):
    """over every rhs the SpTRSM dispatch can see: exactly the 18 compiled instances"""
    got = set()
    for rhs in range(2, 131):
        for args in ((1, 0, rhs, False, 1, 1), (3, 0, rhs, False, 1, 1), (1, 0, rhs, True, 1, 1),
                     (1, 0, rhs, True, 3, 3)):
            S = sb.trsv_shape_host(*args, NCU)
            assert S["rp"] * S["v"] == S["c"] and S["rows_per_claim"] * S["rp"] == 64
            assert S["passes"] == -(-rhs // S["c"])
            got.add((S["rp"], S["v"], S["sys"]))
    assert got == TRIPLES and len(got) == 18


@pytest.mark.parametrize("args", [
    (4, 0, 1, False, 1, 1, NCU), (-1, 0, 1, False, 1, 1, NCU), (1, 0, 0, False, 1, 1, NCU),
    (1, 0, 1, False, 1, 1, 0), (1, 0, 1, True, 0, 0, NCU), (1, 0, 1, True, 2, 3, NCU), (1, 0, 1, True, 2, 0, NCU),
    (1, 0, 1, False, 2, 1, NCU), (0, 0, 1, True, 1, 1, NCU), (2, 0, 1, True, 1, 1, NCU), (3, 0, 1, True, 1, 1, NCU),
    (2, 0, 2, False, 1, 1, NCU), (0, 4, 2, False, 1, 1, NCU), (0, 0, 2, False, 1, 1, NCU), (0, -1, 1, False, 1, 1, NCU)])
def test_rejected(sb, args):
    with pytest.raises(sb.SblasError):
        sb.trsv_shape_host(*args)


# ---- the level analysis and the level-set executor's schedule --------------
def levels(sb, system, sub=0):
    return sb.trsv_levels_host(system[0], system[1], sub)


@pytest.mark.parametrize("sub", [0, 1])
def test_levels_chain(sb, sub):
    want = dict(levels=5000, widest=1, narrow_runs=1, wide_runs=0)
    assert levels(sb, schedule_system("chain", sub), sub) == want
    assert levels(sb, chain_system(5000, sub), sub) == want


@pytest.mark.parametrize("sub,nlev,widest", [(0, 15, 33132), (1, 20, 33292)])
def test_levels_wide(sb, sub, nlev, widest):
    """values computed on the CPU from the generator and its seeds; the wide run is levels 0-3"""
    assert levels(sb, schedule_system("wide", sub), sub) == dict(levels=nlev, widest=widest, narrow_runs=1, wide_runs=1)


def test_narrow_wide_boundary(sb):
    assert levels(sb, one_level_then_row(2048)) == dict(levels=2, widest=2048, narrow_runs=1, wide_runs=0)
    assert levels(sb, one_level_then_row(2049)) == dict(levels=2, widest=2049, narrow_runs=1, wide_runs=1)


def test_three_runs(sb):
    assert levels(sb, three_run_system()) == dict(levels=3, widest=2049, narrow_runs=1, wide_runs=2)


@pytest.mark.parametrize("name", ["qh768", "ash85"])
def test_levels_kat(sb, orc, name):
    cp, ri = kat(name, "fwd")[:2]
    assert sb.trsv_levels_host(cp, ri, 0)["levels"] == orc.levels_lower(cp, ri)


def test_levels_trivial_and_rejected(sb):
    import numpy as np
    assert sb.trsv_levels_host([0, 1], [0], 0) == dict(levels=1, widest=1, narrow_runs=1, wide_runs=0)
    assert sb.trsv_levels_host([0], np.zeros(0, np.int32), 0) == dict(levels=0, widest=0, narrow_runs=0, wide_runs=0)
    for cp, ri, sub in (([0, 1], [1], 0), ([0, 1], [-1], 0), ([0, 2, 1], [0, 1], 0), ([1, 2], [0, 0], 0),
                        ([0, 1], [0], 2)):
        with pytest.raises(sb.SblasError):
            sb.trsv_levels_host(cp, ri, sub)
