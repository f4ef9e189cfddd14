"""The premises of tests/exact_inputs.py, proved without a GPU: with integers for the linear layers and with the CPU checker alone for
the grid scatter.  The GPU modules test_gpu_exact_linear.py and test_gpu_exact_grid_scatter.py ask the kernels for bit equality; that is
only fair while every partial sum is exact in f32, which is what fails here when a generator is changed carelessly (for example q = 7
in three dimensions: 26 bits)."""
import numpy as np
import pytest

import exact_inputs as E
from oracle import oracle as O


def _every_case():
    for K, N in E.LINEAR_SHAPES:
        for M in E.LINEAR_BATCHES:
            yield M, K, N
    yield E.M_PAST_FORWARD_CAP, 36, 64
    yield E.M_PAST_GRAD_W_CAP, 36, 64


# ---- linear -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
def test_linear_sums_stay_below_2_to_24(relu):
    for M, K, N in _every_case():
        x, w, gy = E.linear_case(M, K, N)
        for a in (x, w, gy):
            assert a.dtype == np.float32 and np.array_equal(a, np.rint(a))
        budget = E.linear_budget(x, w, gy, relu)
        for name, v in budget.items():
            assert v < E.LIMIT, (M, K, N, name, v)
    assert 4 * E.M_PAST_GRAD_W_CAP < E.LIMIT
    assert E.M_PAST_FORWARD_CAP > 2048 * 4 * 16 and E.M_PAST_GRAD_W_CAP > 1536 * 4 * 8 * 16
    assert E.M_PAST_FORWARD_CAP % 16 == 5 and E.M_PAST_GRAD_W_CAP % 16 == 5


def test_linear_reference_is_the_int64_product():
    """the float64 route of exact_inputs._exact_matmul against numpy's own int64 matmul, at the sizes where that is quick"""
    for K, N in E.LINEAR_SHAPES:
        x, w, gy = E.linear_case(63, K, N)
        xi, wi, gi = (np.rint(a).astype(np.int64) for a in (x, w, gy))
        for relu in (False, True):
            r = E.linear_reference(x, w, gy, relu)
            pre = xi @ wi.T
            gm = gi * (pre > 0) if relu else gi
            assert np.array_equal(r["pre"], pre) and np.array_equal(r["y"], np.maximum(pre, 0) if relu else pre)
            assert np.array_equal(r["dx"], gm @ wi) and np.array_equal(r["dw"], gm.T @ xi)
            z = E.as_f32(r["dx"])
            assert z.dtype == np.float32 and (z == 0).any() and not np.signbit(z[z == 0]).any()     # the zeros asked for are +0


def test_linear_outputs_sit_on_both_sides_of_the_kink_and_on_it():
    for K, N in E.LINEAR_SHAPES:
        x, w, gy = E.linear_case(5003, K, N)
        pre = E.linear_reference(x, w, gy, True)["pre"]
        zero, pos, neg = (pre == 0).mean(), (pre > 0).mean(), (pre < 0).mean()
        assert zero >= 0.05 and pos >= 0.2 and neg >= 0.2, (K, N, zero, pos, neg)
        assert (pre == 0).all(1).any() and (pre == 0).all(0).any() == (N > 2)     # whole rows and (N > 2) a whole column of y == 0
        # gradients arrive at the y == 0 elements: the mask rule is exercised, not vacuous
        assert (gy[pre == 0] != 0).mean() > 0.5


# ---- MLP --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", E.MLP_BATCHES)
def test_mlp_chain_stays_below_2_to_24_at_every_layer(M):
    x, ws, g = E.mlp_case(M)
    for w in ws:
        assert set(np.unique(w)) == {-1.0, 0.0, 1.0}
    r = E.mlp_reference(x, ws, g)
    assert r["budget"] < E.LIMIT, r["budget"]
    # nothing degenerate: every layer's output, every weight gradient and the input gradient have plenty of nonzeros, and the hidden
    # pre-activations hit 0 as well as both signs
    for a in r["acts"][1:]:
        assert (a != 0).mean() > 0.2
    for dw in r["dws"]:
        assert (dw != 0).mean() > 0.1
    assert (r["dx"] != 0).mean() > 0.2
    assert M > 2048 * 4 * 16 or M == 5003


# ---- grid -------------------------------------------------------------------------------------------------------------------------
def _checker(name, x, g):
    from lzzx_nerf_amd.gridencoder import GridEncoder
    enc = GridEncoder(**E.grid_kwargs(name))
    D, L, C, H, T, gt, _ = E.GRID_CASES[name]
    assert enc.per_level_scale == 2.0
    off = O.grid_offsets(D, L, 2.0, H, T)
    assert np.array_equal(off, enc.offsets.numpy())
    ge, _ = O.grid_encode_backward(g, x, tuple(enc.embeddings.shape), off, 2.0, H, None, 0 if gt == "hash" else 1)
    return ge


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _grid_premises(name, B, q=None):
    """returns the list of premises that fail (empty when all hold)"""
    D = E.GRID_CASES[name][0]
    q_ = E.GRID_CASES[name][6] if q is None else q
    unit = 2.0 ** -(D * q_)
    x, g = E.grid_inputs(name, B, q)
    ge = _checker(name, x, g)
    failed = []
    if not np.array_equal(_bits(ge), _bits(_checker(name, x[::-1], g[::-1]))):
        failed.append("reversal")
    perm = np.random.default_rng(B).permutation(B)
    if not np.array_equal(_bits(ge), _bits(_checker(name, x[perm], g[perm]))):
        failed.append("permutation")
    scaled = ge.astype(np.float64) / unit
    if not np.array_equal(scaled, np.rint(scaled)):
        failed.append("multiple of the unit")
    mass = _checker(name, x, np.abs(g)).astype(np.float64)
    if not mass.max() < E.LIMIT * unit:
        failed.append("bit budget")
    assert (ge != 0).any() and (mass == 0).any()
    return failed


@pytest.mark.parametrize("name,B", [(n, B) for n in E.GRID_CASES for B in E.GRID_BATCHES[n]])
def test_grid_scatter_is_exact_in_any_order(name, B):
    D, q = E.GRID_CASES[name][0], E.GRID_CASES[name][6]
    x, g = E.grid_inputs(name, B)
    k = x.astype(np.float64) * (1 << q)
    assert np.array_equal(k, np.rint(k)) and x.min() == 0.0 and x.max() == 1.0
    assert not x[0].any() and (x[1] == 1).all() and (x[10:50] == x[10]).all()
    assert np.array_equal(g, np.rint(g)) and g.min() == -8 and g.max() == 8
    assert E.grid_unit(name) == 2.0 ** -(D * q)
    assert _grid_premises(name, B) == []


def test_q7_in_three_dimensions_breaks_the_premise():
    """the reason the generator keeps q = 5 for D = 3: 21 fractional bits leave no room for the sums"""
    failed = _grid_premises("D3C2T16", 70001, q=7)
    assert "permutation" in failed or "bit budget" in failed, failed


def test_uniform_random_inputs_do_depend_on_the_order():
    """the checker's sum is not order-blind by construction: ordinary inputs change bits under the same permutation"""
    name, B = "D3C2T16", 4099
    rng = np.random.default_rng(1)
    D, L, C = E.GRID_CASES[name][:3]
    x, g = rng.random((B, D)).astype(np.float32), rng.normal(size=(B, L * C)).astype(np.float32)
    perm = rng.permutation(B)
    assert not np.array_equal(_bits(_checker(name, x, g)), _bits(_checker(name, x[perm], g[perm])))


# ---- three planes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", sorted(E.PLANE_CONFIGS))
@pytest.mark.parametrize("bound", E.PLANE_BOUNDS)
def test_plane_scatter_is_exact_in_any_order(config, bound):
    from lzzx_nerf_amd.gridencoder import GridEncoder
    enc = GridEncoder(input_dim=2, level_dim=1, **E.PLANE_CONFIGS[config])
    assert enc.per_level_scale == 2.0 and enc.num_levels == 4
    kw = E.PLANE_CONFIGS[config]
    off = O.grid_offsets(2, 4, 2.0, kw["base_resolution"], kw["log2_hashmap_size"])
    assert np.array_equal(off, enc.offsets.numpy())
    shape = tuple(enc.embeddings.shape)
    for B in E.PLANE_BATCHES:
        xyz, g = E.plane_inputs(B, bound)
        unit01 = O.map01(xyz, bound)
        k = unit01.astype(np.float64) * (1 << E.PLANE_Q)
        inside = (unit01 >= 0) & (unit01 <= 1)
        assert np.array_equal(k[inside], np.rint(k[inside])) and (~inside).sum() == 3
        assert np.array_equal(np.abs(xyz[[0, 1]]), np.full((2, 3), bound, np.float32))
        perm = np.random.default_rng(B).permutation(B)
        for p, cols in enumerate(E.PLANE_COLUMNS):
            uv, gp = unit01[:, cols], g[:, 4 * p:4 * p + 4]
            run = lambda u, v: O.grid_encode_backward(v, u, shape, off, 2.0, kw["base_resolution"], None, 0)[0]
            ge = run(uv, gp)
            assert np.array_equal(_bits(ge), _bits(run(uv[::-1], gp[::-1]))) and np.array_equal(_bits(ge), _bits(run(uv[perm], gp[perm])))
            scaled = ge.astype(np.float64) / E.PLANE_UNIT
            assert np.array_equal(scaled, np.rint(scaled))
            assert run(uv, np.abs(gp)).astype(np.float64).max() < E.LIMIT * E.PLANE_UNIT, (config, bound, B, p)
