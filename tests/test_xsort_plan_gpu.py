"""The plan a handle builds is the plan sblas.xsort_plan_host returns: the
exported planner entry is what build_xsort_plan actually uses.

resident is the device's CU count: the kernel's LDS use (over 128 KiB of a
CU's 160 KiB) admits one workgroup per CU; if the occupancy query of the plan
build ever said otherwise, `grid` would disagree here.
"""
import numpy as np
import pytest

from test_xsort_devplan_gpu import MATRICES, OPT_IDS, OPTS
from test_xsort_plan_cpu import WRANGE

pytestmark = pytest.mark.gpu

XSORT = 5


@pytest.mark.parametrize("opts", OPTS, ids=OPT_IDS)
@pytest.mark.parametrize("name", ["ragged", "mostly_empty", "unit_rows"])
def test_handle_plan_is_host_plan(torch_cuda, sb, name, opts):
    n, rp, col, val = MATRICES[name](np.random.default_rng(2024))
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    p = sb.xsort_plan_host(rp, n, cus, **{k[3:]: v for k, v in opts.items()})
    with sb.test_options(**opts):
        A = sb.DeviceCSR.upload(0, n, rp, col, val)
        A.analyse(XSORT)
    try:
        info = A.xsort_info()
        xrec, wranges, heads = (A.xsort_export(w) for w in (1, 2, 3))
    finally:
        A.close()
    assert (info["ready"], info["ranges"], info["wide"], info["items"], info["grid"], info["solo"]) == \
        (1, p["nranges"], p["nwide"], p["nitems"], p["grid"], p["solo"])
    R = p["ranges"]
    wr = np.zeros(p["nwide"], WRANGE)
    for j, f in enumerate(WRANGE.names):
        wr[f] = R[R[:, 2] == 1, j]
    assert np.array_equal(wr.view(np.uint8), wranges)
    # words 0-3 of the record of every (queue, index, team) slot
    sub = np.full((8, p["qstride"], 2), -1, np.int64)
    for k, q in enumerate(p["queues"]):
        sub[k, :len(q)] = q
    sub = sub.ravel()
    want = np.full((len(sub), 4), -1, np.int64)
    want[:, 0] = sub
    live = sub >= 0
    r = R[sub[live] >> 8]
    want[live, 1] = (r[:, 0] & 0xffffffff) | (r[:, 1] << 32)
    want[live, 2] = r[:, 4]
    want[live, 3] = r[:, 3]
    got = xrec.view(np.int64).reshape(len(sub), p["G"] + 5)[:, :4]
    assert np.array_equal(got, want)
    want_heads = np.zeros(32, np.int32)
    want_heads[0:8] = want_heads[16:24] = p["qstat"]
    assert np.array_equal(heads.view(np.int32), want_heads)
