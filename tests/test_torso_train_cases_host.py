"""The inputs of tests/test_gpu_torso_train_branches.py (tests/torso_train_cases.py), without a device: they are the regimes they
claim to be, the float32 restatement of the model stays within a quarter of every bound against float64, and a model with one branch of
the backward wrong (clamp gate, alpha path of the mix, the - bg term, the mask) misses the right one by at least ten bounds.

One condition cannot hold as the others do.  In the few-pixel size cases (N <= 257) the table gradient of a fine level is one
pixel's corner weight times a number of the tensor's own maximum, and the weight carries the rounding of pos = fma(u, 2047, 0.5) to
f32: half an ulp at 2^11 is 6e-5 of a cell, 0.3 bounds, in ANY f32 evaluation.  The restatement measures 0.34-0.66 bounds there, and
0.15-0.22 from N = 3000 up, where the coarse levels' sums set the maximum.  For those cases the table is held to the bound itself,
every other tensor to the quarter."""
import functools

import pytest
import torch

import torso_train_cases as T

CASES = dict(T.gpu_cases())
FEW = 1000   # below this many pixels the table gradient's maximum is a single pixel's


@functools.lru_cache(maxsize=None)
def _ref(name):
    return T.run_model(CASES[name])


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_are_the_regime(name):
    c = CASES[name]
    _, d = _ref(name)
    assert c.rejected <= 0.02 * c.drawn, (c.rejected, c.drawn)
    assert float(d["min_pre"].min()) > T.PRE_MARGIN
    assert float((d["v"].abs() - 1).abs().min()) > T.CLAMP_MARGIN
    assert float(T.cell_margin(c.sd, d["v"]).min()) > T.CELL_MARGIN
    cl = T.clamp_classes(d["v"], c.mask)
    live = c.N if c.mask is None else int(c.mask.sum())
    if c.mask is not None:
        assert float((d["occupancy"] - T.GRID_THRESH).abs().min()) > T.OCC_MARGIN
        assert torch.equal(d["occupancy"] > T.GRID_THRESH, c.mask)
        assert 0.2 <= live / c.N <= 0.8
    if c.regime == "C" and c.N >= FEW:
        assert min(int(cl[k].sum()) for k in ("both", "only0", "only1")) >= 16, {k: int(v.sum()) for k, v in cl.items()}
        assert int(cl["none"].sum()) >= live / 2
        assert not bool(c.gd.any())
    if c.regime != "C":
        assert int(cl["none"].sum()) == live
    # f32 takes every ReLU and the clamp on the float64 side
    _, d32 = T.run_model(c, torch.float32)
    assert torch.equal(d32["branches"], d["branches"])


@pytest.mark.parametrize("name", list(CASES))
def test_f32_restatement_within_a_quarter_of_the_bounds(name):
    c = CASES[name]
    ref, _ = _ref(name)
    got, _ = T.run_model(c, torch.float32)
    r = T.ratios(got, ref, c)
    print(name, {k: "%.3f" % v for k, v in r.items()})
    for k in c.keys:
        assert float(ref[k].abs().max()) > 0, (name, k)          # a relative bound needs a scale
        limit = 1.0 if (k == "torso_encoder.embeddings" and c.N < FEW) else 0.25
        assert r[k] <= limit, (name, k, r[k])


def _applies(name, variant):
    c = CASES[name]
    if variant == "no_clamp_gate":
        return c.regime == "C" and c.N >= FEW
    if variant == "mask_ignored":
        return c.mask is not None
    return c.bg is not None and c.regime != "C"


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_a_wrong_branch_misses_by_ten_bounds(variant):
    names = [n for n in CASES if _applies(n, variant)]
    assert names
    for name in names:
        c = CASES[name]
        ref, _ = _ref(name)
        wrong, _ = T.run_model(c, torch.float64, variant)
        r = T.ratios(wrong, ref, c)
        print(variant, name, {k: "%.1f" % v for k, v in r.items()})
        assert max(r.values()) >= 10, (variant, name, r)


def test_the_clamp_gate_reaches_every_deform_gradient_in_regime_c():
    """with a zero upstream deform gradient a missing gate moves every deform-net weight gradient by more than 100 bounds"""
    for name in ("C-ind0-nomix", "C-ind8-mix"):
        c = CASES[name]
        r = T.ratios(T.run_model(c, torch.float64, "no_clamp_gate")[0], _ref(name)[0], c)
        assert min(r[k] for k in T.DEFORM_KEYS) >= 100, r


@pytest.mark.parametrize("ind_dim", [0, 8])
@pytest.mark.parametrize("only", ["both", "only0", "only1"])
def test_exact_zeros_of_the_clamp_in_the_model(ind_dim, only):
    """what the GPU test's exact part expects, in float64: upstream gradients on the pixels clamped in both coordinates alone leave
    the deform net without gradient; on those clamped in coordinate d alone, row d of the last deform layer"""
    c = T.case_c(ind_dim, True, only=only)
    assert int((c.ga[:, 0] != 0).sum()) >= 16
    g, _ = T.run_model(c)
    assert bool(g["torso_net.net.0.weight"].any()) and bool(g["torso_net.net.2.weight"].any())
    w2 = g["torso_deform_net.net.2.weight"]
    if only == "both":
        assert not any(bool(g[k].any()) for k in T.DEFORM_KEYS)
    else:
        d = 0 if only == "only0" else 1
        assert not bool(w2[d].any()) and bool(w2[1 - d].any())


def test_occupancy_is_grid_sample():
    import torch.nn.functional as Fn
    grid = torch.from_numpy(T.blob())
    xy = torch.cat([T.case_f(8, "tensor", True).xy, torch.tensor([[1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [0.0, 0.0]])])
    want = Fn.grid_sample(grid.double().view(1, 1, T.GRID_G, T.GRID_G), xy.double().view(1, -1, 1, 2), align_corners=True).view(-1)
    assert float((torch.from_numpy(T.occupancy(grid, T.GRID_G, xy)) - want).abs().max()) < 1e-14
