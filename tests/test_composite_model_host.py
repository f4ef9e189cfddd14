"""The float64 model of training compositing (tests/composite_cases.py) and the CPU checker against it.

* the model against closed forms: a one-sample and a two-sample ray, the unweighted ambient sum, a ray that terminates early;
* the model's autograd gradients against central differences of its own float64 forward -- the model is a derivative, not a second
  restatement of the kernel's backward formula;
* the checker (the hand restatement of raymarching.cu:603-809 every device kernel is bit-pinned to) against the model: every case, every
  variant, every output and every gradient array per element, early termination, dropped and empty rays, chunk-edge counts and non-zero
  counter bases included.  This is where the bars of the device tests come from (MEASURED / BARS in composite_cases.py)."""
import numpy as np
import pytest
import torch

import composite_cases as C
from oracle import oracle as O


def _checker(variant, case):
    """the checker's forward and backward on a case; upstream grad_depth has no entry in its backward (raymarching.py:323)"""
    na, aw, hu = C.VARIANTS[variant]
    a1, un = (case["amb1"] if na > 1 else None), (case["unc"] if hu else None)
    fwd = O.composite_rays_train_forward(variant, case["sigma"], case["rgb"], case["deltas"], case["rays"], case["amb0"], a1, un,
                                         T_thresh=case["T_thresh"])
    g = dict(grad_weights_sum=case["g_weights_sum"], grad_image=case["g_image"], grad_amb0_sum=case["g_amb0_sum"])
    if na > 1:
        g["grad_amb1_sum"] = case["g_amb1_sum"]
    if hu:
        g["grad_unc_sum"] = case["g_unc_sum"]
    bwd = O.composite_rays_train_backward(variant, g, case["sigma"], case["rgb"], case["deltas"], case["rays"], fwd, case["amb0"], a1, un,
                                          T_thresh=case["T_thresh"])
    return fwd, bwd


def _tiny(rays, M, sigma, dt, T_thresh=1e-4, seed=0):
    rng = np.random.default_rng(seed)
    t = 2.0 + np.cumsum(dt)
    return C.case_from_arrays("tiny", rays, M, sigma, np.stack([dt, t], 1), rng.uniform(0, 1, (M, 3)), rng.uniform(0, 1, M),
                              rng.uniform(0, 1, M), rng.uniform(0, 1, M), T_thresh, rng)


def _f64(case, k):
    return case[k].astype(np.float64)


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
def test_model_one_sample_ray():
    """w = alpha = 1 - exp(-sigma dt); d w / d sigma = dt exp(-sigma dt)"""
    case = _tiny([[0, 0, 1]], 1, np.array([30.0]), np.array([0.02]))
    m = C.model64("triplane", case)
    s, dt, t = _f64(case, "sigma")[0], _f64(case, "deltas")[0, 0], _f64(case, "deltas")[0, 1]
    w = 1 - np.exp(-s * dt)
    out, g = m["out"], m["grads"]
    assert out["weights_sum"][0] == pytest.approx(w, rel=1e-14) and out["depth"][0] == pytest.approx(w * t, rel=1e-14)
    assert np.allclose(out["image"][0], w * _f64(case, "rgb")[0], rtol=1e-14, atol=0)
    assert out["amb0_sum"][0] == _f64(case, "amb0")[0] and out["amb1_sum"][0] == _f64(case, "amb1")[0]
    assert out["unc_sum"][0] == pytest.approx(w * _f64(case, "unc")[0], rel=1e-14)
    dw = dt * np.exp(-s * dt)
    up = _f64(case, "g_weights_sum")[0] + _f64(case, "g_image")[0] @ _f64(case, "rgb")[0] + _f64(case, "g_unc_sum")[0] * _f64(case, "unc")[0]
    assert g["grad_sigmas"][0] == pytest.approx(dw * up, rel=1e-12)
    assert np.allclose(g["grad_rgbs"][0], w * _f64(case, "g_image")[0], rtol=1e-14, atol=0)
    assert g["grad_amb0"][0] == _f64(case, "g_amb0_sum")[0] and g["grad_amb1"][0] == _f64(case, "g_amb1_sum")[0]
    assert g["grad_unc"][0] == pytest.approx(w * _f64(case, "g_unc_sum")[0], rel=1e-14)
    # the `sigma` variant weights the ambient channel by w
    ms = C.model64("sigma", case)
    assert ms["out"]["amb0_sum"][0] == pytest.approx(w * _f64(case, "amb0")[0], rel=1e-14)
    assert ms["grads"]["grad_amb0"][0] == pytest.approx(w * _f64(case, "g_amb0_sum")[0], rel=1e-14)
    up_s = _f64(case, "g_weights_sum")[0] + _f64(case, "g_image")[0] @ _f64(case, "rgb")[0] + _f64(case, "g_amb0_sum")[0] * _f64(case, "amb0")[0]
    assert ms["grads"]["grad_sigmas"][0] == pytest.approx(dw * up_s, rel=1e-12)
    assert ms["grads"]["grad_amb1"] is None and ms["grads"]["grad_unc"] is None and not m["near"].any()


def test_model_two_sample_ray():
    """w0 = a0, w1 = a1 (1 - a0): the first sample's sigma moves both weights, the second's only its own; ray id 1 of 2, ray 0 empty"""
    case = _tiny([[1, 0, 2], [0, 2, 0]], 2, np.array([20.0, 45.0]), np.array([0.01, 0.025]))
    m = C.model64("uncertainty", case)
    s, dl, rgb, unc = _f64(case, "sigma"), _f64(case, "deltas"), _f64(case, "rgb"), _f64(case, "unc")
    e = np.exp(-s * dl[:, 0])
    a = 1 - e
    w = np.array([a[0], a[1] * e[0]])
    out, g = m["out"], m["grads"]
    assert out["weights_sum"][1] == pytest.approx(w.sum(), rel=1e-14) and out["weights_sum"][0] == 0.0
    assert np.allclose(out["image"][1], w @ rgb, rtol=1e-14, atol=0) and not out["image"][0].any()
    assert out["depth"][1] == pytest.approx(w @ dl[:, 1], rel=1e-14) and out["amb0_sum"][1] == pytest.approx(_f64(case, "amb0").sum(), rel=1e-15)
    gw, gi, gu = _f64(case, "g_weights_sum")[1], _f64(case, "g_image")[1], _f64(case, "g_unc_sum")[1]
    up = gw + rgb @ gi + gu * unc                            # d loss / d w_k
    # d w0 / d s0 = dt0 e0, d w1 / d s0 = -dt0 e0 a1, d w1 / d s1 = dt1 e1 e0
    assert g["grad_sigmas"][0] == pytest.approx(dl[0, 0] * e[0] * (up[0] - a[1] * up[1]), rel=1e-12)
    assert g["grad_sigmas"][1] == pytest.approx(dl[1, 0] * e[1] * e[0] * up[1], rel=1e-12)
    assert np.allclose(g["grad_rgbs"], w[:, None] * gi[None, :], rtol=1e-14, atol=0)
    assert np.allclose(g["grad_unc"], w * gu, rtol=1e-14, atol=0) and np.all(g["grad_amb0"] == _f64(case, "g_amb0_sum")[1])


def test_model_terminated_ray_and_unweighted_ambient_sum():
    """six samples, sigma dt = 5 each: T = e^-5, e^-10 < 1e-4 -- the second sample crosses the threshold and is included, the four behind it
    get zero weight and zero gradient, the unweighted ambient sum is the plain sum of the two visited values; a dropped ray gives zeros"""
    M = 9
    case = _tiny([[0, 0, 6], [1, 6, 4]], M, np.full(M, 250.0), np.full(M, 0.02))
    rgb, a0, a1, dl = _f64(case, "rgb"), _f64(case, "amb0"), _f64(case, "amb1"), _f64(case, "deltas")
    for variant in C.VARIANTS:
        m = C.model64(variant, case)
        out, g = m["out"], m["grads"]
        x = float(_f64(case, "sigma")[0] * dl[0, 0])              # 5 to float32 rounding of dt
        w = np.array([1 - np.exp(-x), np.exp(-x) * (1 - np.exp(-x))])
        assert out["weights_sum"][0] == pytest.approx(w.sum(), rel=1e-12) and out["weights_sum"][0] == pytest.approx(1 - np.exp(-2 * x), rel=1e-12)
        assert np.allclose(out["image"][0], w @ rgb[:2], rtol=1e-12, atol=0) and out["depth"][0] == pytest.approx(w @ dl[:2, 1], rel=1e-12)
        if variant == "sigma":
            assert out["amb0_sum"][0] == pytest.approx(w @ a0[:2], rel=1e-12)
        else:
            assert out["amb0_sum"][0] == a0[0] + a0[1]
            assert np.all(g["grad_amb0"][:2] == _f64(case, "g_amb0_sum")[0])
        if variant == "triplane":
            assert out["amb1_sum"][0] == a1[0] + a1[1] and np.all(g["grad_amb1"][:2] == _f64(case, "g_amb1_sum")[0])
        for k, v in g.items():
            if v is not None:
                assert not v[2:].any(), (variant, k)            # behind the stop, and the dropped ray's rows (6 + 4 > 9)
        assert g["grad_sigmas"][:2].all() and g["grad_rgbs"][:2].all()
        for k, v in out.items():
            if v is not None:
                assert not np.asarray(v[1]).any(), (variant, k)  # the dropped ray
        assert not m["near"].any()


def test_model_marks_a_ray_that_stops_next_to_the_threshold():
    """sigma dt chosen so that T after the second sample is T_thresh (1 + 5e-4): inside the band, marked; at (1 + 5e-3): outside, not"""
    for rel, marked in ((5e-4, True), (5e-3, False), (-5e-4, True)):
        x = -np.log(1e-4 * (1 + rel)) / 2
        case = _tiny([[0, 0, 3]], 3, np.full(3, x / 0.02), np.full(3, 0.02))
        # (float32 sigma moves T by ~1e-7 relative: far inside either side of the band)
        assert bool(C.model64("ambient", case)["near"][0]) == marked


# ---- the model is a derivative ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
@pytest.mark.parametrize("name", ["n65_b200_drop", "n130_b0_drop", "n65_b200_tail_T0"])
def test_model_gradients_equal_central_differences_of_its_forward(variant, name):
    """a handful of elements of each of the five inputs, on rays not in `near`: rows in front of a stop, the row that stops a ray, rows
    behind it (zero), rows of dropped rays and rows no ray owns (zero)"""
    case = C.CASES[name]
    m = C.model64(variant, case)
    na, aw, hu = C.VARIANTS[variant]
    rng = np.random.default_rng(5)
    ok_rows = np.nonzero(~m["near_row"])[0]
    live = ok_rows[m["visited"][ok_rows]]
    rows = np.concatenate([rng.choice(live, 5, replace=False), rng.choice(ok_rows, 3, replace=False)])
    base = C.inputs64(case)

    def loss(which, row, col, h):
        x = [b.clone() for b in base]
        if col is None:
            x[which][row] += h
        else:
            x[which][row, col] += h
        with torch.no_grad():
            return float(C.loss64(variant, case, C.forward64(variant, case, *x)[0]))

    names = ["grad_sigmas", "grad_rgbs", "grad_amb0", "grad_amb1", "grad_unc"]
    nonzero = 0
    for which, key in enumerate(names):
        got = m["grads"][key]
        if got is None:
            continue
        for row in rows:
            col = int(rng.integers(3)) if key == "grad_rgbs" else None
            h = 1e-6
            fd = (loss(which, row, col, h) - loss(which, row, col, -h)) / (2 * h)
            g = got[row] if col is None else got[row, col]
            assert g == pytest.approx(fd, rel=1e-6, abs=1e-8), (key, int(row), g, fd)
            nonzero += g != 0
    assert nonzero >= 3 * (2 + na + hu)                  # (five visited rows per input; a sample of sigma 0 has weight 0 and no colour gradient)


# ---- the checker against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_near_threshold_share_is_under_the_cap(name):
    case = C.CASES[name]
    for variant in C.VARIANTS:
        near = C.model64(variant, case)["near"]
        assert near.sum() <= C.NEAR_CAP * case["N"], (variant, int(near.sum()))


def test_cases_hold_what_they_are_meant_to():
    for name, case in C.CASES.items():
        rays = case["rays"].astype(np.int64)
        N, M = case["N"], case["M"]
        assert sorted(rays[:, 0]) == list(range(N)) and rays[0, 1] == case["base"]
        assert (rays[1:, 1] == rays[:-1, 1] + rays[:-1, 2]).all()
        fits = rays[:, 1] + rays[:, 2] <= M
        if N > 3:
            assert set(C.EDGE_COUNTS) <= set(rays[:, 2]) and not (rays[:, 0] == np.arange(N)).all()
            inner = rays[1:-1, 2]
            assert (inner == 0).any()                                      # an empty ray inside a group
        if case["ending"] == "tail":
            assert fits.all() and M == rays[-1, 1] + rays[-1, 2] + C.TAIL
        else:
            first = int(np.argmin(fits))
            assert (0 < first or N == 3) and first <= N - 3 and not fits[first:].any() and fits[:first].all()
            assert rays[first, 1] < M < rays[first, 1] + rays[first, 2]    # M lands inside a ray's range
        assert M <= 3000
        if N > 3:
            assert 0.1 < (case["sigma"][case["owner"] >= 0] == 0).mean() < 0.3   # a fifth of the sigmas exactly 0
    assert not C.CASES["n3_b200_all_dropped"]["kept"].any() and C.CASES["n3_b200_all_dropped"]["M"] == 204
    one = C.CASES["n1_b200_tail"]
    assert one["rays"].tolist() == [[0, 200, 9]] and one["M"] == 209 + C.TAIL
    t0 = C.CASES["n65_b200_tail_T0"]
    assert t0["T_thresh"] == 0.0 and (t0["sigma"] == 1e4).sum() == 12
    m = C.model64("triplane", t0)
    assert (m["out"]["weights_sum"] == 1.0).sum() >= 5                     # T reached exactly 0 ...
    assert m["visited"][t0["owner"] >= 0].all()                            # ... and the walk went on over every sample
    # about half the rays of the thresholded cases stop early
    for name in ("n130_b200_tail", "n64_b200_tail"):
        c = C.CASES[name]
        vis = C.model64("ambient", c)["visited"]
        cut = [not vis[o:o + n].all() for _, o, n in c["rays"][c["kept"]]]
        assert 0.3 < np.mean(cut) < 0.8


def test_checker_is_within_the_recorded_bars_of_the_model(capsys):
    """every case x variant x quantity per element; prints the measured table (pytest -s) that MEASURED in composite_cases.py records"""
    worst = {k: 0.0 for k in C.MEASURED}
    scale = {k: 0.0 for k in C.MEASURED}
    for name, case in C.CASES.items():
        for variant in C.VARIANTS:
            m = C.model64(variant, case)
            fwd, bwd = _checker(variant, case)
            want, got = C.quantities(variant, m["out"], m["grads"]), C.quantities(variant, fwd, bwd)
            assert set(want) == set(got)
            for k in want:
                assert np.isfinite(got[k]).all()
                d = C.max_abs_diff(got[k], want[k], m["near_id"] if k in C.PER_RAY else m["near_row"])
                assert d <= C.BARS[k], (name, variant, k, d, C.BARS[k])
                worst[k], scale[k] = max(worst[k], d), max(scale[k], float(np.abs(want[k]).max(initial=0)))
            # rows no ray owns, rows behind a stop, rows of dropped rays: exactly zero
            for k in ("grad_sigmas", "grad_rgbs", "grad_amb0", "grad_amb1", "grad_unc"):
                if bwd[k] is not None:
                    assert not bwd[k][~m["visited"] & ~m["near_row"]].any(), (name, variant, k)
                    assert not m["grads"][k][~m["visited"]].any()
        go, gd = O.march_rays_train_backward(case["g_xyzs"], case["g_dirs"], case["rays"], case["deltas"])
        wo, wd = C.march_backward64(case)
        for k, got, want in (("grad_rays_o", go, wo), ("grad_rays_d", gd, wd)):
            d = C.max_abs_diff(got, want)
            assert d <= C.BARS[k], (name, k, d, C.BARS[k])
            worst[k], scale[k] = max(worst[k], d), max(scale[k], float(np.abs(want).max()))
            assert not got[~case["kept"]].any()
    with capsys.disabled():
        print("\nchecker vs float64 model, max |diff| over all cases and variants (value magnitude):")
        for k in C.MEASURED:
            print(f'    "{k}": {worst[k]!r},    # magnitude {scale[k]:.3g}')
    for k in C.MEASURED:
        assert C.BARS[k] <= C.BAR_FACTOR * C.MEASURED[k]                       # no bar wider than 4 x the measurement it was set from ...
        assert C.MEASURED[k] <= worst[k] * (1 + 1e-6), (k, C.MEASURED[k], worst[k])   # ... and the record is what this run measures
