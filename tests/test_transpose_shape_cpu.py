"""The transpose's pass shape on the CPU (sblas.transpose_shape_host: no GPU):
which form every named case of the GPU tests takes on a 256-CU device, that
together they take every form the library has, and the config-2 shape."""
import pytest

from transpose_cases import CASES, EDGES, MGPU_CASES, transpose_case, transpose_edge

NCU = 256

# case -> (msd, c, bA, bB, pack, ftile, lean) or (lsd, passes, rb, ntiles)
FORMS = {
    "qh768": ("msd", 8, 1, 1, 8, 3072, 0),
    "ash85": ("lsd", 1, 7, 1),
    "random": ("msd", 7, 3, 2, 7, 3072, 1),
    "longcols": ("msd", 1, 3, 2, 1, 4096, 0),
    "wide": ("msd", 8, 5, 4, 8, 3072, 0),
    "big": ("msd", 8, 7, 7, 8, 3072, 0),
    "shortrows": ("msd", 6, 4, 3, 6, 3072, 1),
    "sparserows": ("msd", 8, 8, 8, 8, 3072, 0),
    "hugecols": ("lsd", 4, 7, 5),
    "narrow2tiles": ("lsd", 2, 5, 2),
    "manyrows": ("msd", 8, 3, 2, -1, 3072, 0),
}


def shape_of(sb, m, n, rp):
    return sb.transpose_shape_host(m, n, int(rp[-1]), NCU)


def form_of(T):
    if T["msd"]:
        return ("msd", T["c"], T["bA"], T["bB"], T["pack"], T["ftile"], T["lean"])
    return ("lsd", T["passes"], T["rb"], T["ntiles"])


@pytest.fixture(scope="module")
def shapes(sb):
    out = {}
    for case in CASES:
        m, n, rp, _, _ = transpose_case(sb, case, seed=5)
        out[case] = shape_of(sb, m, n, rp)
    return out


@pytest.mark.parametrize("case", CASES)
def test_case_form(shapes, case):
    assert form_of(shapes[case]) == FORMS[case]


@pytest.mark.parametrize("case", MGPU_CASES)
def test_mgpu_case_form(sb, case):
    """the whole matrix of a multi-device case (the ngpu = 1 block)"""
    m, n, rp, _, _ = transpose_case(sb, case, seed=11)
    assert form_of(shape_of(sb, m, n, rp)) == FORMS[case]


@pytest.mark.parametrize("shape", EDGES)
def test_edge_form(sb, shape):
    m, n, rp, _, _ = transpose_edge(shape)
    assert form_of(shape_of(sb, m, n, rp)) == ("msd", 8, 3, 2, 8, 3072, 0)


def test_cases_cover_every_form(shapes):
    T = list(shapes.values())
    msd = [t for t in T if t["msd"]]
    lsd = [t for t in T if not t["msd"]]
    assert any(t["passes"] == 1 for t in lsd)                       # LSD, one pass
    assert any(t["passes"] > 1 and t["ntiles"] > 1 for t in lsd)    # LSD, several passes and tiles
    assert any(t["bB"] <= 7 for t in msd)                           # pass B, 128 digits
    assert any(t["bB"] == 8 for t in msd)                           # pass B, 256 digits
    assert any(t["pack"] >= 0 for t in msd) and any(t["pack"] < 0 for t in msd)
    assert any(t["ftile"] == 3072 for t in msd) and any(t["ftile"] == 4096 for t in msd)
    assert any(t["lean"] for t in msd) and any(not t["lean"] for t in msd)
    assert shapes["big"]["S"] > 1                                   # more than one tile per workgroup
    # consistency of every shape
    for t in T:
        assert t["nwg"] == -(-t["ntiles"] // t["S"]) and t["nwg"] <= 2 * NCU
        if t["msd"]:
            assert 1 <= t["bA"] <= 8 and 1 <= t["bB"] <= 8 and 1 <= t["c"] <= 8
            assert t["nbC"] == 1 << (t["bA"] + t["bB"]) and t["nwgB"] == t["JB"] << t["bA"]
            assert t["fgrid"] == min(t["nbC"], NCU * (3 if t["lean"] else 2))
            assert not t["lean"] or (t["pack"] >= 0 and t["c"] <= 7 and t["ftile"] == 3072)
        else:
            assert 1 <= t["rb"] <= 8 and t["ncnt"] == t["nwg"] << t["rb"]


def test_config2_shape(sb):
    T = sb.transpose_shape_host(2_000_000, 2_000_000, 39_750_000, NCU)
    assert form_of(T) == ("msd", 7, 7, 7, 7, 3072, 1)
    assert (T["S"], T["nwg"]) == (19, 511)
    assert (T["JB"], T["nwgB"], T["packA"], T["nbC"], T["fgrid"]) == (4, 512, 14, 16384, 768)


def test_rejects_bad_arguments(sb):
    with pytest.raises(sb.SblasError):
        sb.transpose_shape_host(10, 10, 5, 0)
    with pytest.raises(sb.SblasError):
        sb.transpose_shape_host(-1, 10, 5, 256)
