"""Row split, XCD panels and CSR5 on the small matrices of spmv_cases.py, each
chosen for one path of the kernels.  Every case asserts, in this order: the
path that ran (sblas_csr_spmv_info against literal counts), that the handle's
counts are the host functions' answer for the same rowptr(s), y bit for bit
against the vectors the library produced before the experiment forms were
removed (golden/spmv_forms/, where that form was recorded), and the oracle's
per-row bound, for beta = 0 (y0 seeded with NaN) and beta != 0."""
import os

import numpy as np
import pytest

import spmv_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_REF = {}


def reference(orc, name, beta):
    """the oracle's y and per-row bound of a case, computed once"""
    if (name, beta) not in _REF:
        c = sc.gpu_case(name)
        y0 = np.zeros(c["m"]) if beta == 0.0 else c["y0"]
        args = (c["rp"], c["col"], c["val"], c["x"].copy(), sc.ALPHA, beta, y0)
        _REF[(name, beta)] = (orc.csr_spmv(*args), orc.spmv_bound(*args))
    return _REF[(name, beta)]


def run_and_check(torch, sb, orc, name, algo, opts, golden):
    """both betas through one form; returns the handle's info"""
    c = sc.gpu_case(name)
    info = None
    for beta, key in ((0.0, "y_beta0"), (sc.BETA, "y_beta")):
        got, info = sc.run_case(torch, sb, c, algo, opts, beta)
        if golden:
            want = np.load(os.path.join(GOLDEN, "spmv_forms", f"{name}-{golden}.npz"))[key]
            assert np.array_equal(got, want), f"{name}-{golden} {key}: {np.sum(got != want)} rows differ"
        ref, bound = reference(orc, name, beta)
        err = np.abs(got - ref)
        assert np.all(err <= bound), f"beta {beta}: max excess {np.max(err - bound)} at {np.argmax(err - bound)}"
    return info


def host_blocks(sb, rowptrs):
    tot = {k: 0 for k in sb.ROWSPLIT_BLOCK_KEYS}
    for rp in rowptrs:
        h = sb.rowsplit_blocks_host(rp)
        for k in tot:
            tot[k] = max(tot[k], h[k]) if k == "max_rows" else tot[k] + h[k]
    return tot


def host_tiles(sb, rowptrs):
    tot = dict(tiles=0, gap_tiles=0, seg_rows=0, empty_rows=0)
    for rp in rowptrs:
        h = sb.csr5_plan_host(rp)
        for k, hk in zip(tot, ("tiles", "gap_tiles", "seg_rows", "n_empty")):
            tot[k] += h[hk]
    return tot


# the row blocks each case is there for (plain row split)
ROWSPLIT_PATH = {f"rows{k}": dict(blocks=1, stream=1, max_rows=k) for k in sc.STREAM_ROWS}
ROWSPLIT_PATH.update({
    "block2048": dict(blocks=2, stream=2, max_rows=7),
    "unaligned": dict(blocks=2, stream=2, max_rows=6),
    "long2049": dict(blocks=1, stream=0, long1=1, longn=0),
    "long2049_off": dict(blocks=3, stream=2, long1=1, longn=0),
    "long8192": dict(blocks=2, stream=1, long1=1, longn=0, slots=0),
    "long8193": dict(blocks=2, stream=0, long1=0, longn=1, slots=2),
    "two_long": dict(blocks=8, stream=3, long1=0, longn=2, slots=5),
    "empty_block": dict(blocks=2, stream=2, max_rows=1024),
    "c5_ends": dict(stream=2, long1=0, longn=0, max_rows=1024),
    "c5_gap": dict(blocks=1, stream=1, max_rows=405),
    "c5_pad_inf": dict(blocks=3, stream=2, long1=1),
    "first_third": dict(blocks=5, stream=2, long1=1, longn=1, slots=2),
})
assert set(ROWSPLIT_PATH) == set(sc.GPU_CASES)


@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_rowsplit(torch_cuda, sb, orc, name):
    info = run_and_check(torch_cuda, sb, orc, name, sb.ROWSPLIT, {}, "rowsplit")
    assert info["panels"] == 0 and info["psplit"] == 0
    assert {k: info[k] for k in ROWSPLIT_PATH[name]} == ROWSPLIT_PATH[name]
    assert {k: info[k] for k in sb.ROWSPLIT_BLOCK_KEYS} == host_blocks(sb, [sc.gpu_case(name)["rp"]])


PANEL_FORMS = {"panel2": (4, {"panels": 2}), "panel3": (4, {"panels": 3}),
               "rowsplit_panel2": (1, {"rs_panel": 1, "panels": 2}),
               "rowsplit_panel3": (1, {"rs_panel": 1, "panels": 3})}


@pytest.mark.parametrize("form", PANEL_FORMS)
@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_panels(torch_cuda, sb, orc, name, form):
    """The columns leave the middle third of x unused: 2 of 3 panels are live
    (and both of 2).  The row split over panels is the panel plan, so both
    must give the parent's panel3 vector.  first_third has one live panel:
    the plain row split runs, and gives the plain row split's vector."""
    algo, opts = PANEL_FORMS[form]
    psplit = opts["panels"]
    c = sc.gpu_case(name)
    degenerate = name == "first_third"
    golden = ("rowsplit" if degenerate else "panel3") if psplit == 3 else None
    info = run_and_check(torch_cuda, sb, orc, name, algo, opts, golden)
    if degenerate:
        assert info["panels"] == 0 and info["psplit"] == 0
        assert {k: info[k] for k in ROWSPLIT_PATH[name]} == ROWSPLIT_PATH[name]
        assert {k: info[k] for k in sb.ROWSPLIT_BLOCK_KEYS} == host_blocks(sb, [c["rp"]])
        return
    assert info["panels"] == 2 and info["psplit"] == psplit
    rps = sc.panel_rowptrs(c, psplit)
    assert len(rps) == 2
    assert {k: info[k] for k in sb.ROWSPLIT_BLOCK_KEYS} == host_blocks(sb, rps)
    # a long row's entries fall into the two live panels: the halves of 2049 are stream rows, those of
    # 8192 / 8193 / 9000 single chunks, the larger half of 16385 keeps two chunks
    want_long = {"long2049": dict(stream=2, long1=0), "long8192": dict(long1=2, longn=0),
                 "long8193": dict(long1=2, longn=0), "two_long": dict(long1=3, longn=1, slots=2)}
    if name in want_long:
        assert {k: info[k] for k in want_long[name]} == want_long[name]


# the tiles each CSR5 case is there for (plain form)
CSR5_PATH = {
    "c5_ends": dict(tiles=3, gap_tiles=0, seg_rows=0, empty_rows=0),        # 301 and 1024 row ends, no gap
    "c5_gap": dict(tiles=2, gap_tiles=2, seg_rows=202, empty_rows=203),     # 201 row ends in a gap tile
    "c5_pad_inf": dict(tiles=4, gap_tiles=1, seg_rows=3, empty_rows=1),
    "rows1024": dict(tiles=2, gap_tiles=1, empty_rows=1),
    "empty_block": dict(tiles=1, gap_tiles=1, seg_rows=3, empty_rows=1025),
    "two_long": dict(tiles=25, gap_tiles=1, seg_rows=2, empty_rows=1),
}
CSR5_FORMS = {"csr5": {}, "csr5_hostplan": {"csr5_hostplan": 1}, "csr5_panel2": {"csr5_panel": 1, "panels": 2},
              "csr5_panel3": {"csr5_panel": 1, "panels": 3}}


@pytest.mark.parametrize("form", CSR5_FORMS)
@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_csr5(torch_cuda, sb, orc, name, form):
    opts = CSR5_FORMS[form]
    c = sc.gpu_case(name)
    psplit = opts.get("panels", 0)
    plain = psplit == 0 or name == "first_third"  # one live panel: the plain form
    golden = form if form != "csr5_panel2" else None
    info = run_and_check(torch_cuda, sb, orc, name, sb.CSR5, opts, golden)
    counts = {k: info[k] for k in ("tiles", "gap_tiles", "seg_rows", "empty_rows")}
    if plain:
        assert info["panels"] == 0 and info["psplit"] == 0
        if name in CSR5_PATH:
            assert {k: info[k] for k in CSR5_PATH[name]} == CSR5_PATH[name]
        assert counts == host_tiles(sb, [c["rp"]])
    else:
        assert info["panels"] == 2 and info["psplit"] == psplit
        assert counts == host_tiles(sb, sc.panel_rowptrs(c, psplit))


def test_first_third_is_one_vector(sb):
    """with one live panel every row-split form is the plain row split, every CSR5 form the plain CSR5"""
    def load(form):
        z = np.load(os.path.join(GOLDEN, "spmv_forms", f"first_third-{form}.npz"))
        return z["y_beta0"], z["y_beta"]
    for a, b in (("rowsplit", "panel3"), ("csr5", "csr5_panel3"), ("csr5", "csr5_hostplan")):
        for u, v in zip(load(a), load(b)):
            assert np.array_equal(u, v)


def test_spmv_info_needs_a_plan(torch_cuda, sb):
    c = sc.gpu_case("rows4")
    A = sb.DeviceCSR.upload(0, c["n"], c["rp"], c["col"], c["val"])
    try:
        for algo in (sb.ROWSPLIT, sb.CSR5, 3, sb.PANEL):
            with pytest.raises(sb.SblasError):
                A.spmv_info(algo)
        A.analyse(sb.CSR5)
        assert A.spmv_info(3) == A.spmv_info(sb.CSR5)  # 3 is the same plan
        with pytest.raises(sb.SblasError):
            A.spmv_info(sb.ROWSPLIT)
        A.analyse(sb.XSORT)
        for algo in (sb.AUTO, sb.XSORT, 6):
            with pytest.raises(sb.SblasError):
                A.spmv_info(algo)
    finally:
        A.close()
