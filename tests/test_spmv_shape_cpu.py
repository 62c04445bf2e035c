"""What the row-split, CSR5 and XCD-panel SpMV decide on the host (no GPU):
AUTO's pick and the panel rule on both sides of every threshold, the row
blocks of literal rowptrs, CSR5's tile descriptors against a numpy
restatement (cases in spmv_cases.py)."""
import numpy as np
import pytest

import spmv_cases as sc


@pytest.mark.parametrize("args,want", sc.PICK_CASES, ids=[str(i) for i in range(len(sc.PICK_CASES))])
def test_pick(sb, args, want):
    got = sb.spmv_shape_host(0, 10, **args)
    assert got["algo"] == want
    assert got["wants_probe"] == 1  # AUTO always looks at the columns


@pytest.mark.parametrize("algo,args,want", sc.PANEL_CASES, ids=[str(i) for i in range(len(sc.PANEL_CASES))])
def test_panels(sb, algo, args, want):
    got = sb.spmv_shape_host(algo, 10, **args)
    assert {k: got[k] for k in want} == want


def test_shape_reads_no_process_state(sb, monkeypatch):
    """the environment and the test hooks are the caller's to pass in"""
    monkeypatch.setenv("SBLAS_AUTO", "2")
    with sb.test_options(rs_panel=1, csr5_panel=1, panels=5, csr5_hostplan=1):
        assert sb.spmv_shape_host(0, 10, n=1000, nnz=1000, share=0.125)["algo"] == 4
        assert sb.spmv_shape_host(1, 10, n=1000, nnz=10) == dict(algo=1, panels=0, npanels=1, W=1000, c5_host=0,
                                                                 wants_probe=0)
        assert sb.spmv_shape_host(2, 10, n=1000, nnz=10)["c5_host"] == 0


def test_shape_bad_arguments(sb):
    for bad in (dict(algo=-1), dict(algo=6), dict(m=-1), dict(n=-1), dict(nnz=-1)):
        a = dict(algo=1, m=1, n=1, nnz=1)
        a.update(bad)
        with pytest.raises(sb.SblasError):
            sb.spmv_shape_host(a["algo"], a["m"], n=a["n"], nnz=a["nnz"])


@pytest.mark.parametrize("name", sc.ROWBLOCK_CASES)
def test_row_blocks(sb, name):
    lens, blocks, counts = sc.ROWBLOCK_CASES[name]
    got = sb.rowsplit_blocks_host(sc.rowptr_of(lens))
    assert got["list"].tolist() == blocks
    assert tuple(got[k] for k in sb.ROWSPLIT_BLOCK_KEYS) == counts


def test_row_blocks_bad_rowptr(sb):
    for rp in ([1, 2], [0, 3, 2], [0, 1 << 31]):
        with pytest.raises(sb.SblasError):
            sb.rowsplit_blocks_host(rp)
        with pytest.raises(sb.SblasError):
            sb.csr5_plan_host(rp)


def _csr5_rowptrs():
    out = {f"c5_{k}": (lambda v=v: sc.rowptr_of(v)) for k, v in sc.CSR5_LENS.items()}
    out.update({f"gpu_{k}": (lambda v=v: sc.rowptr_of(v)) for k, v in sc.GPU_LENS.items()})
    for gen in (sc.ragged, sc.empty_runs, sc.tile_rows):
        out[gen.__name__] = lambda gen=gen: gen(np.random.default_rng(11))[2]
    return out


CSR5_ROWPTRS = _csr5_rowptrs()


@pytest.mark.parametrize("name", CSR5_ROWPTRS)
def test_csr5_descriptors(sb, name):
    rp = CSR5_ROWPTRS[name]()
    got, want = sb.csr5_plan_host(rp), sc.csr5_brute(rp)
    for k in ("flags", "seg_off", "seg_row", "empty_rows", "head_run"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["tile_row"].view(np.uint32), want["tile_row"])
    gaps = int(np.sum(want["tile_row"][:-1] >> 31))
    assert (got["tiles"], got["gap_tiles"], got["seg_rows"], got["n_empty"]) == (
        len(want["head_run"]), gaps, len(want["seg_row"]), len(want["empty_rows"]))
    assert got["head_runs"] == int(np.sum(want["head_run"] > 0))
    assert got["longest_run"] == int(want["head_run"].max(initial=0))


def test_csr5_literals(sb):
    """a few descriptors by hand, so that the restatement is pinned too"""
    p = sb.csr5_plan_host(sc.rowptr_of(sc.CSR5_LENS["row3000"]))  # rows start at entries 0, 5, 3005
    assert (p["tiles"], p["gap_tiles"], p["head_runs"], p["longest_run"]) == (3, 0, 1, 2)
    assert p["tile_row"].tolist() == [0, 1, 1, 3] and p["head_run"].tolist() == [0, 2, 0]
    assert p["flags"][0] == 0b100001 and p["flags"][2 * 64 + 957 // 16] == 1 << (957 % 16)
    p = sb.csr5_plan_host(sc.rowptr_of(sc.CSR5_LENS["empty_across_edge"]))  # starts 0, 1020 | 1024, 1031
    assert (p["tiles"], p["gap_tiles"], p["seg_rows"], p["n_empty"]) == (2, 1, 2, 3)
    assert p["tile_row"].view(np.uint32).tolist() == [0, 4 | 0x80000000, 7]
    assert p["seg_off"].tolist() == [0, 0, 2] and p["seg_row"].tolist() == [4, 6]
    assert p["empty_rows"].tolist() == [2, 3, 5]
    p = sb.csr5_plan_host(sc.rowptr_of(sc.CSR5_LENS["ones1024"]))
    assert np.all(p["flags"] == 0xffff) and p["tile_row"].tolist() == [0, 1024]
