"""Training compositing on the device, both sample layouts, against the CPU checker (bit for bit) and the float64 autograd model.

The cases, the model and the bars are tests/composite_cases.py's: chunk-edge sample counts, empty rays inside groups, counter bases of 0
and 200, a tail of unowned rows or a dropped suffix, early termination on about half the rays, one ray that is first and last at once,
and T_thresh = 0 with opaque samples.  The bars are the CHECKER's measured distance from the model (test_composite_model_host.py), times 4:
the kernels run the checker's operation sequence, so that distance is theirs too.

* ray-major kernels: bit-equal to the checker, every element within the bar of the model;
* step-major kernels on the permuted rows: per-ray outputs bit-equal to ray-major; the gradient buffers, poisoned with NaN before the
  call, hold the ray-major value at every mapped row and exactly 0 everywhere else -- the kernel writes every row itself;
* the public autograd functions under both layouts: gradients reach every per-sample input and equal the model, grad_depth changes
  nothing, deltas and rays get none;
* the march's backward under both layouts against grad_o = sum g_xyz, grad_d = sum (t g_xyz + g_dirs)."""
import functools

import numpy as np
import pytest
import torch

import composite_cases as C
from test_composite_model_host import _checker

pytestmark = pytest.mark.gpu

GRAD_KEYS = ("grad_sigmas", "grad_rgbs", "grad_amb0", "grad_amb1", "grad_unc")
OUT_KEYS = ("weights_sum", "amb0_sum", "amb1_sum", "unc_sum", "depth", "image")


@functools.lru_cache(maxsize=None)
def _dev(name):
    """a case's arrays on the device, ray-major rows, and once more permuted to step-major rows (unowned rows zero)"""
    case = C.CASES[name]
    dev = torch.device("cuda")
    d = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in case.items() if isinstance(v, np.ndarray) and v.dtype != bool and k != "owner"}
    src, dst = C.step_rows(case["rays"], case["M"])
    d["src"], d["dst"] = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    for k in ("sigma", "rgb", "amb0", "amb1", "unc", "deltas", "g_xyzs", "g_dirs"):
        s = torch.zeros_like(d[k])
        s[d["dst"]] = d[k][d["src"]]
        d[k + "_step"] = s
    assert len(np.unique(dst)) == len(dst) == int(case["rays"][case["kept"], 2].sum())
    return d


def _args(variant, d, step):
    na, aw, hu = C.VARIANTS[variant]
    sfx = "_step" if step else ""
    return (d["sigma" + sfx], d["rgb" + sfx], d["amb0" + sfx], d["amb1" + sfx] if na > 1 else None, d["unc" + sfx] if hu else None,
            d["deltas" + sfx])


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _run(variant, name, layout, monkeypatch=None):
    """forward and backward through the *_v entries; layout 1 on the step-major rows, its gradient buffers NaN before the call"""
    from lzzx_nerf_amd import raymarching as R
    case, d = C.CASES[name], _dev(name)
    v = C.VARIANTS[variant]
    na, aw, hu = v
    sig, rgb, a0, a1, un, dl = _args(variant, d, layout == 1)
    fwd = R._composite_train_fwd(v, sig, rgb, a0, a1, un, dl, d["rays"], case["T_thresh"], layout)
    ws, a0s, a1s, us, dep, img = fwd
    if layout == 1:      # the wrapper hands the step-major kernel torch.empty_like buffers: poison what it gets
        monkeypatch.setattr(torch, "empty_like", lambda t, **kw: torch.full_like(t, float("nan")))
    bwd = R._composite_train_bwd(v, d["g_weights_sum"], d["g_amb0_sum"], d["g_amb1_sum"] if na > 1 else None, d["g_unc_sum"] if hu else None,
                                 d["g_image"], sig, rgb, a0, a1, un, dl, d["rays"], ws, a0s, us, img, case["T_thresh"], layout)
    if layout == 1:
        monkeypatch.undo()
    torch.cuda.synchronize()
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def _ray_major(variant, name):
    return _run(variant, name, 0)


def _within_bars(variant, name, out, grads, what):
    """every element of every quantity within the recorded bar of the model; rays in `near` left out, but finite"""
    m = C.model64(variant, C.CASES[name])
    want, got = C.quantities(variant, m["out"], m["grads"]), C.quantities(variant, out, grads)
    assert set(want) == set(got)
    for k in want:
        assert np.isfinite(got[k]).all(), (what, k)
        d = C.max_abs_diff(got[k], want[k], m["near_id"] if k in C.PER_RAY else m["near_row"])
        print(f"{what} {variant} {name} {k}: max |diff| {d:.3g}, bar {C.BARS[k]:.3g}")
        assert d <= C.BARS[k], (what, variant, name, k, d, C.BARS[k])


@pytest.mark.parametrize("name", C.CASE_NAMES)
@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_ray_major_equals_the_checker_and_the_model(variant, name):
    case = C.CASES[name]
    fwd, bwd = _ray_major(variant, name)
    cf, cb = _checker(variant, case)
    out, grads = {k: _np(t) for k, t in zip(OUT_KEYS, fwd)}, {k: _np(t) for k, t in zip(GRAD_KEYS, bwd)}
    for k in OUT_KEYS:
        assert (out[k] is None) == (cf[k] is None), k
        if out[k] is not None:
            assert np.array_equal(out[k], cf[k]), (k, float(np.abs(out[k] - cf[k]).max()))
    for k in GRAD_KEYS:
        assert (grads[k] is None) == (cb[k] is None), k
        if grads[k] is not None:
            assert np.array_equal(grads[k], cb[k]), (k, float(np.abs(grads[k] - cb[k]).max()))
    _within_bars(variant, name, out, grads, "ray-major")


@pytest.mark.parametrize("name", C.CASE_NAMES)
@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_step_major_writes_every_row_and_equals_the_model(variant, name, monkeypatch):
    case, d = C.CASES[name], _dev(name)
    f_r, b_r = _ray_major(variant, name)
    f_s, b_s = _run(variant, name, 1, monkeypatch)
    for k, x, y in zip(OUT_KEYS, f_r, f_s):
        assert (x is None) == (y is None), k
        if x is not None:
            assert torch.equal(x, y), k
    unowned = torch.ones(case["M"], dtype=torch.bool, device=d["src"].device)
    unowned[d["dst"]] = False
    back = {}
    for k, x, y in zip(GRAD_KEYS, b_r, b_s):
        assert (x is None) == (y is None), k
        if x is None:
            back[k] = None
            continue
        bad = torch.isnan(y).reshape(case["M"], -1).any(1)
        assert not bad.any(), f"{k}: rows {torch.nonzero(bad).flatten().tolist()[:8]}... ({int(bad.sum())} of {case['M']}) were never written"
        assert not y[unowned].any(), k                       # a row no kept ray owns: exactly 0
        z = torch.zeros_like(x)
        z[d["dst"]] = x[d["src"]]
        assert torch.equal(z, y), k                          # a mapped row: the ray-major value (0 behind a stop)
        r = torch.zeros_like(y)
        r[d["src"]] = y[d["dst"]]
        back[k] = _np(r)                                     # back in ray-major rows for the comparison with the model
    _within_bars(variant, name, {k: _np(t) for k, t in zip(OUT_KEYS, f_s)}, back, "step-major")


# ---- the public autograd functions ----------------------------------------------------------------------------------------------------
def _tagged_rays(case, layout):
    """a `rays` tensor tagged by march_rays_train itself (the attribute compositing reads the layout from), holding the case's table"""
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.synthetic import ones_bitfield
    dev = torch.device("cuda")
    N = case["N"]
    ro = torch.zeros(N, 3, device=dev)
    rd = torch.tensor([[0.0, 0.0, 1.0]], device=dev).repeat(N, 1)
    bits = torch.from_numpy(ones_bitfield()).to(dev)
    nears, fars = torch.full((N,), 0.05, device=dev), torch.full((N,), 1.0, device=dev)
    rays = R.march_rays_train(ro, rd, 1.0, bits, 1, 128, nears, fars, None, -1, False, -1, True, 1 / 256, 4, layout=layout, order=False)[3]
    assert rays.lz_layout == layout and rays.shape == (N, 3)
    rays.copy_(torch.from_numpy(case["rays"]))
    return rays


@pytest.mark.parametrize("name", ["n1_b200_tail", "n65_b200_drop", "n130_b200_tail", "n65_b200_tail_T0"])
@pytest.mark.parametrize("layout", ["ray", "step"])
@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_public_functions_carry_the_gradient(variant, layout, name, monkeypatch):
    from lzzx_nerf_amd import raymarching as R
    case, d = C.CASES[name], _dev(name)
    na, aw, hu = C.VARIANTS[variant]
    step = layout == "step"
    rays = _tagged_rays(case, layout)
    sig, rgb, a0, a1, un, dl = [None if t is None else t.clone().requires_grad_(True) for t in _args(variant, d, step)]
    if variant in ("ambient", "sigma"):
        fn = R.composite_rays_train if variant == "ambient" else R.composite_rays_train_sigma
        ins, outs = [sig, rgb, a0], ("weights_sum", "amb0_sum", "depth", "image")
    elif variant == "uncertainty":
        fn, ins, outs = R.composite_rays_train_uncertainty, [sig, rgb, a0, un], ("weights_sum", "amb0_sum", "unc_sum", "depth", "image")
    else:
        fn, ins, outs = R.composite_rays_train_triplane, [sig, rgb, a0, a1, un], OUT_KEYS
    if step:
        monkeypatch.setattr(torch, "empty_like", lambda t, **kw: torch.full_like(t, float("nan")))
    got = dict(zip(outs, fn(*ins, dl, rays, case["T_thresh"])))
    f_r, b_r = _ray_major(variant, name)
    for k, x in zip(OUT_KEYS, f_r):
        if x is not None:
            assert torch.equal(got[k], x), k
    res = []
    for with_depth in (True, False):
        loss = sum((d["g_" + k] * v).sum() for k, v in got.items() if k != "depth" or with_depth)
        res.append(torch.autograd.grad(loss, ins + [dl], allow_unused=True, retain_graph=True))
    monkeypatch.undo()
    assert res[0][-1] is None and res[1][-1] is None                      # deltas get no gradient
    assert not rays.requires_grad and rays.grad is None and rays.dtype == torch.int32
    grads = dict.fromkeys(GRAD_KEYS)
    keys = {3: GRAD_KEYS[:3], 4: GRAD_KEYS[:3] + GRAD_KEYS[4:], 5: GRAD_KEYS}[len(ins)]
    for k, ga, gb, x in zip(keys, res[0], res[1], ins):
        assert ga is not None and ga.shape == x.shape and not torch.isnan(ga).any(), k
        assert torch.equal(ga, gb), k                                      # a non-zero grad_depth changes nothing
        assert float(ga.abs().max()) > 0, k
        if step:
            r = torch.zeros_like(ga)
            r[d["src"]] = ga[d["dst"]]
            owned = torch.zeros(case["M"], dtype=torch.bool, device=ga.device)
            owned[d["dst"]] = True
            assert not ga[~owned].any(), k
            ga = r
        grads[k] = _np(ga)
    assert float(d["g_depth"].abs().max()) > 0 and float(got["depth"].abs().max()) > 0
    _within_bars(variant, name, {k: _np(got.get(k)) for k in OUT_KEYS}, grads, "public " + layout)


# ---- the march's backward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_march_backward_equals_the_model_in_both_layouts(name):
    """ray-major entry: the reference's kernel writes row n of grad_rays_o / grad_rays_d for rays[n] (raymarching.cu:550-555; its rays[]
    are in ray-id order); the grouped entry writes the row of the ray's ID, which is what a permuted processing order needs.  The case's
    ids are a permutation, so the two are compared through it."""
    from oracle import oracle as O
    from lzzx_nerf_amd._util import call, ptr, stream
    case, d = C.CASES[name], _dev(name)
    N, M = case["N"], case["M"]
    dev = d["rays"].device
    outs = []
    for entry, sfx in (("lz_march_rays_train_backward", ""), ("lz_march_rays_train_backward_grouped", "_step")):
        go, gd = torch.zeros(N, 3, device=dev), torch.zeros(N, 3, device=dev)
        call(entry, ptr(d["g_xyzs" + sfx]), ptr(d["g_dirs" + sfx]), ptr(d["rays"]), ptr(d["deltas" + sfx]), N, M, ptr(go), ptr(gd), stream())
        outs.append((go.cpu().numpy(), gd.cpu().numpy()))
    co, cd = O.march_rays_train_backward(case["g_xyzs"], case["g_dirs"], case["rays"], case["deltas"])
    assert np.array_equal(outs[0][0], co) and np.array_equal(outs[0][1], cd)
    ids = case["rays"][:, 0]
    by_pos = (outs[1][0][ids], outs[1][1][ids])                           # the grouped entry's rows, by position in rays[]
    assert np.array_equal(by_pos[0], outs[0][0]) and np.array_equal(by_pos[1], outs[0][1])
    wo, wd = C.march_backward64(case)
    for what, (go, gd) in (("ray-major", outs[0]), ("step-major", by_pos)):
        for k, got, want in (("grad_rays_o", go, wo), ("grad_rays_d", gd, wd)):
            diff = C.max_abs_diff(got, want)
            print(f"{what} {name} {k}: max |diff| {diff:.3g}, bar {C.BARS[k]:.3g}")
            assert diff <= C.BARS[k], (what, name, k, diff, C.BARS[k])
            assert not got[~case["kept"]].any()                           # an empty or dropped ray gets zero
    assert np.abs(wd).max() > 1 or not case["kept"].any()
