"""tests/golden/reference_objective.npz (the reference's own TrainerUtil.train_step, run by tests/golden/make_golden_objective.py) against
the float64 restatement of tests/objective_spec.py, term by term and gradient by gradient.  CPU only: this pins the specification that
tests/test_gpu_objective.py then holds the kernels to."""
import os

import numpy as np
import pytest
import torch

import objective_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "reference_objective.npz"), allow_pickle=False)
CASES = [str(c) for c in Z["head_cases"]]


def case(name):
    """one case: what the fixture stores, the inputs rebuilt from their hash, zero gradients for inputs the objective did not read"""
    c = {k.split("__", 1)[1]: Z[k] for k in Z.files if k.startswith(name + "__")}
    N, seed = int(c["N"]), int(c["seed"])
    if name == "torso":
        c.update(S.torso_inputs(N, seed))
        return c
    c.update(S.case_inputs(N, seed, str(c["face_mode"]), str(c["bg_mode"]), float(c["image_lo"]), float(c["image_hi"])))
    for k in ("image_raw", "ws", "aud", "eye", "unc"):
        c.setdefault("g_" + k, np.zeros_like(c[k]))
    if bool(c["regularized"]):
        for k in ("unc", "aud", "eye"):
            c.setdefault("g_reg_" + k, np.zeros_like(c["reg_" + k]))
    return c


def head_f64(c):
    """the spec in float64 on the fixture's inputs -> (loss, terms, {leaf: grad}, {reg_k: grad} or None)"""
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    leaves = {k: d(c[k]).requires_grad_(True) for k in ("image_raw", "ws", "aud", "eye", "unc")}
    bg = d(c["bg"]) if c["bg"].ndim else float(c["bg"])
    flags = tuple(bool(f) for f in c["flags"])
    sf = min(int(c["step"]) / int(c["iters"]), 1.0)
    loss, pred, terms = S.head_objective(leaves["image_raw"], leaves["ws"], leaves["aud"], leaves["eye"], leaves["unc"], bg, d(c["target"]),
                                         torch.from_numpy(c["face"]), sf, flags)
    reg = None
    total = loss
    if bool(c["regularized"]):
        raw = [d(c["raw_" + k]) for k in ("unc", "aud", "eye")]
        reg = [d(c["reg_" + k]).requires_grad_(True) for k in ("unc", "aud", "eye")]
        total = loss + S.jitter(raw, reg, sf, flags)
    total.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in leaves.items()}
    greg = None if reg is None else [(r.grad if r.grad is not None else torch.zeros_like(r)).numpy() for r in reg]
    return float(total.detach()), pred.detach().numpy(), np.array([float(terms[k].detach()) for k in S.TERMS]), grads, greg


def _close(got, want, tol, what):
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize("name", CASES)
def test_fixture_equals_the_float64_spec(name):
    c = case(name)
    loss, _, terms, grads, greg = head_f64(c)
    assert abs(float(c["loss"]) - loss) <= 1e-5 * abs(loss), (name, float(c["loss"]), loss)
    for i, k in enumerate(S.TERMS):          # each term against the largest term (a term can be 0 or 1e-9 of the loss)
        assert abs(float(c["terms"][i]) - terms[i]) <= 1e-5 * np.abs(terms).max(), (name, k, float(c["terms"][i]), terms[i])
    for k, g in grads.items():
        _close(c["g_" + k], g, 1e-5, (name, "g_" + k))
    if greg is not None:
        for i, k in enumerate(("unc", "aud", "eye")):
            if np.abs(greg[i]).max() > 0:
                _close(c["g_reg_" + k], greg[i], 1e-5, (name, "g_reg_" + k))
            else:
                assert not np.any(c["g_reg_" + k]), (name, k)


def test_fixture_inputs_are_rebuilt_bit_for_bit():
    """the hash that replaces stored inputs: pinned values, so a change to it cannot pass silently against a fixture made with another"""
    h = S.hash_unit(0, 1, (6,))
    assert h.dtype == np.float32 and (h * 256).astype(int).tolist() == [201, 218, 18, 96, 168, 186]
    assert np.array_equal(S.hash_unit(7, 3, (4, 3)), S.hash_unit(7, 3, (12,)).reshape(4, 3))
    c = case("step1")
    assert abs(float(c["loss"])) > 0 and (c["image_raw"] < 0).any() and (c["image_raw"] > 1).any()


def test_fixture_covers_the_cases_the_spec_names():
    steps = {int(case(n)["step"]) for n in CASES}
    assert {1, 300, 200000, 400000} <= steps and any(s % 16 == 0 and s < 200000 for s in steps)
    flags = {tuple(bool(f) for f in case(n)["flags"]) for n in CASES}
    assert {(True, True, True), (False, True, True), (True, True, False), (True, False, False)} <= flags
    faces = [case(n)["face"] for n in CASES]
    assert any(f.all() for f in faces) and any(not f.any() for f in faces) and any(0 < f.mean() < 1 for f in faces)
    assert {int(case(n)["N"]) for n in CASES} >= {1, 4097}
    assert any(case(n)["bg"].ndim == 0 for n in CASES) and any(case(n)["bg"].ndim == 2 for n in CASES)
    assert any(bool(case(n)["regularized"]) for n in CASES)
    ws = np.concatenate([case(n)["ws"] for n in CASES])
    assert (ws == 0).any() and (ws == 1).any()
    img = np.concatenate([case(n)["image_raw"].ravel() for n in CASES])
    assert (img < 0).any() and (img > 1).any()


def test_torso_fixture_equals_the_float64_spec():
    c = case("torso")
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    color, anchors = d(c["torso_color"]).requires_grad_(True), d(c["anchor_points"]).requires_grad_(True)
    loss = S.torso_objective(color, d(c["target"]), anchors)
    loss.backward()
    assert abs(float(c["loss"]) - float(loss)) <= 1e-5 * abs(float(loss))
    _close(c["g_torso_color"], color.grad.numpy(), 1e-5, "g_torso_color")
    _close(c["g_anchor_points"], anchors.grad.numpy(), 1e-5, "g_anchor_points")
