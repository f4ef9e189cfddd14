"""The fused training objective (lzzx_nerf_amd/objective.py, csrc/lz_objective.hip) against the reference's own train_step
(tests/golden/reference_objective.npz) and the float64 restatement (tests/objective_spec.py); bits across calls, GradScaler, no host
synchronisation, argument errors; and one `-O` training step with the fused objective against the same step on the torch restatement."""
import numpy as np
import pytest
import torch

import objective_spec as S
from test_objective_reference import CASES, case

pytestmark = pytest.mark.gpu

KEYS = ("image_raw", "ws", "aud", "eye", "unc")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _run_fused(c, scaler=None):
    """the fixture case through HeadObjective (+ jitter_regularizer) -> (loss, pred, terms, {leaf: grad}, [g_reg] or None)"""
    from lzzx_nerf_amd.objective import HeadObjective, jitter_regularizer
    flags = tuple(bool(f) for f in c["flags"])
    obj = HeadObjective(int(c["iters"]), unc_loss=flags[0], amb_aud_loss=flags[1], amb_eye_loss=flags[2])
    leaves = {k: _dev(c[k]).requires_grad_(True) for k in KEYS}
    bg = _dev(c["bg"]) if c["bg"].ndim else float(c["bg"])
    step = int(c["step"])
    loss, pred, terms = obj(leaves["image_raw"], leaves["ws"], leaves["aud"], leaves["eye"], leaves["unc"], bg, _dev(c["target"]),
                            _dev(c["face"]), step)
    total, reg = loss, None
    if bool(c["regularized"]):
        assert obj.wants_regularizer(step)
        raw = [_dev(c["raw_" + k]) for k in ("unc", "aud", "eye")]
        reg = [_dev(c["reg_" + k]).requires_grad_(True) for k in ("unc", "aud", "eye")]
        total = loss + jitter_regularizer(raw, reg, obj.step_factor(step), obj.regularizer_flags())
    (scaler.scale(total) if scaler is not None else total).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    greg = None if reg is None else [(r.grad if r.grad is not None else torch.zeros_like(r)) for r in reg]
    return total.detach(), pred, terms, grads, greg


def _close(got, want, tol, what):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize("name", CASES)
def test_head_objective_matches_the_reference_and_the_spec(name):
    from test_objective_reference import head_f64
    c = case(name)
    loss, pred, terms, grads, greg = _run_fused(c)
    torch.cuda.synchronize()
    # against the reference's train_step (f32 torch on the CPU)
    assert abs(float(loss) - float(c["loss"])) <= 1e-5 * abs(float(c["loss"])), (name, float(loss), float(c["loss"]))
    tscale = np.abs(c["terms"]).max()
    for i, k in enumerate(S.TERMS):
        assert abs(float(terms[i]) - float(c["terms"][i])) <= 1e-5 * tscale, (name, k)
    for k in KEYS:
        _close(grads[k], c["g_" + k], 1e-5, (name, "g_" + k))
    # against the float64 restatement
    l64, p64, t64, g64, gr64 = head_f64(c)
    _close(pred, p64, 1e-6, (name, "pred"))
    assert abs(float(loss) - l64) <= 1e-6 * abs(l64), (name, float(loss), l64)
    for i, k in enumerate(S.TERMS):
        assert abs(float(terms[i]) - t64[i]) <= 1e-6 * np.abs(t64).max(), (name, k, float(terms[i]), t64[i])
    for k in KEYS:
        _close(grads[k], g64[k], 1e-6, (name, "g_" + k, "f64"))
    if greg is not None:
        for i, k in enumerate(("unc", "aud", "eye")):
            _close(greg[i], c["g_reg_" + k], 1e-5, (name, "g_reg_" + k))
            if np.abs(gr64[i]).max() > 0:
                _close(greg[i], gr64[i], 1e-6, (name, "g_reg_" + k, "f64"))


def test_torso_objective_matches_the_reference():
    from lzzx_nerf_amd.objective import TorsoObjective
    c = case("torso")
    color, anchors = _dev(c["torso_color"]).requires_grad_(True), _dev(c["anchor_points"]).requires_grad_(True)
    loss, terms = TorsoObjective()(color, _dev(c["target"]), anchors)
    loss.backward()
    assert abs(float(loss) - float(c["loss"])) <= 1e-5 * abs(float(c["loss"]))
    assert abs(float(terms.sum()) - float(loss)) <= 1e-6 * float(loss)
    _close(color.grad, c["g_torso_color"], 1e-5, "g_torso_color")
    _close(anchors.grad, c["g_anchor_points"], 1e-5, "g_anchor_points")


def _big_case(N, seed=0, flags=(True, True, True), step=96000, M=None):
    g = np.random.default_rng(seed)
    u = lambda *s: g.random(s, dtype=np.float32)
    c = dict(image_raw=u(N, 3) * 1.2 - 0.1, ws=u(N), aud=u(N) * 4, eye=u(N) * 16, unc=u(N) * 3, target=u(N, 3), face=u(N) < 0.4,
             bg=u(N, 3), step=np.int64(step), iters=np.int64(200000), flags=np.array(flags), regularized=np.bool_(M is not None))
    c["ws"][:2] = (0.0, 1.0)
    if M is not None:
        for k in ("unc", "aud", "eye"):
            c["raw_" + k] = u(M, 1)
            c["reg_" + k] = c["raw_" + k] + (u(M, 1) - 0.5) * 1e-2
    return c


@pytest.mark.parametrize("N", [65536, 262144])
def test_large_batches_match_the_float64_spec(N):
    from test_objective_reference import head_f64
    c = _big_case(N, M=N * 4)
    loss, pred, terms, grads, greg = _run_fused(c)
    l64, p64, t64, g64, gr64 = head_f64(c)
    assert abs(float(loss) - l64) <= 1e-6 * abs(l64), (float(loss), l64)
    for i, k in enumerate(S.TERMS):
        assert abs(float(terms[i]) - t64[i]) <= 1e-6 * np.abs(t64).max(), (k, float(terms[i]), t64[i])
    _close(pred, p64, 1e-6, "pred")
    for k in KEYS:
        _close(grads[k], g64[k], 1e-6, "g_" + k)
    for i in range(3):
        _close(greg[i], gr64[i], 1e-6, ("g_reg", i))


def test_same_bits_on_every_call():
    c = _big_case(100000, seed=3, M=300000)
    a, b = _run_fused(c), _run_fused(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in KEYS:
        assert torch.equal(a[3][k], b[3][k]), k
    for x, y in zip(a[4], b[4]):
        assert torch.equal(x, y)


def test_grad_scaler_scales_the_gradients_exactly():
    c = _big_case(5000, seed=4, M=9000)
    _, _, _, g1, r1 = _run_fused(c)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    _, _, _, g2, r2 = _run_fused(c, scaler=scaler)
    for k in KEYS:
        assert torch.equal(g2[k], g1[k] * 2.0 ** 16), k
    for x, y in zip(r1, r2):
        assert torch.equal(y, x * 2.0 ** 16)


def test_no_host_synchronisation_and_autocast():
    c = _big_case(4096, seed=5, M=8192)
    from lzzx_nerf_amd.objective import HeadObjective, jitter_regularizer
    obj = HeadObjective(200000)
    leaves = {k: _dev(c[k]).requires_grad_(True) for k in KEYS}
    args = (_dev(c["bg"]), _dev(c["target"]), _dev(c["face"]), 96000)
    raw = [_dev(c["raw_" + k]) for k in ("unc", "aud", "eye")]
    reg = [_dev(c["reg_" + k]).requires_grad_(True) for k in ("unc", "aud", "eye")]
    obj(leaves["image_raw"], leaves["ws"], leaves["aud"], leaves["eye"], leaves["unc"], *args)   # workspace allocated outside the check
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            loss, _, _ = obj(leaves["image_raw"], leaves["ws"], leaves["aud"], leaves["eye"], leaves["unc"], *args)
            loss = loss + jitter_regularizer(raw, reg, obj.step_factor(96000), obj.regularizer_flags())
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and torch.isfinite(loss)
    assert all(torch.isfinite(v.grad).all() for v in leaves.values())


def test_value_errors():
    from lzzx_nerf_amd.objective import HeadObjective, TorsoObjective, jitter_regularizer
    N = 64
    x = {k: torch.rand(N, device="cuda") for k in ("ws", "aud", "eye", "unc")}
    img, tgt, face = torch.rand(N, 3, device="cuda"), torch.rand(N, 3, device="cuda"), torch.rand(N, device="cuda") < 0.5
    obj = HeadObjective(1000)
    loss, pred, terms = obj(img[None], x["ws"][None], x["aud"][None], x["eye"][None], x["unc"][None], 1.0, tgt[None], face[None].to(torch.uint8), 5)
    assert pred.shape == (1, N, 3) and terms.shape == (6,)
    e = torch.empty(0, device="cuda")
    with pytest.raises(ValueError):
        obj(torch.empty(0, 3, device="cuda"), e, e, e, e, 1.0, torch.empty(0, 3, device="cuda"), torch.empty(0, dtype=torch.bool, device="cuda"), 5)
    with pytest.raises(ValueError):       # mismatched shapes
        obj(img[:-1], x["ws"], x["aud"], x["eye"], x["unc"], 1.0, tgt, face, 5)
    with pytest.raises(ValueError):
        obj(img, x["ws"], x["aud"][:-1], x["eye"], x["unc"], 1.0, tgt, face, 5)
    with pytest.raises(ValueError):       # B > 1
        obj(img.view(2, N // 2, 3), x["ws"].view(2, -1), x["aud"].view(2, -1), x["eye"].view(2, -1), x["unc"].view(2, -1), 1.0,
            tgt.view(2, N // 2, 3), face.view(2, -1), 5)
    with pytest.raises(ValueError):
        obj(img, x["ws"], x["aud"], x["eye"], x["unc"], 1.0, tgt, face.float(), 5)
    with pytest.raises(ValueError):
        HeadObjective(1000, amb_aud_loss=False, amb_eye_loss=True)
    with pytest.raises(ValueError):
        HeadObjective(1000, patch_size=2)
    with pytest.raises(ValueError):
        TorsoObjective()(img, tgt[:-1], torch.rand(3, 4, device="cuda"))
    with pytest.raises(ValueError):
        TorsoObjective()(torch.empty(0, 3, device="cuda"), torch.empty(0, 3, device="cuda"), torch.rand(3, 4, device="cuda"))
    with pytest.raises(ValueError):
        jitter_regularizer((x["unc"], x["aud"], x["eye"]), (x["unc"], x["aud"][:-1], x["eye"]), 0.5, (True, True, True))
    with pytest.raises(ValueError):
        jitter_regularizer((e, e, e), (e, e, e), 0.5, (True, True, True))


@pytest.mark.parametrize("arr", ["f32", "O"])
def test_training_step_with_the_fused_objective(params, golden, arr):
    """one training step (arr "O": the f16 head arrangement of `-O` training, loss scaled by 2^16 as its GradScaler does): march_rays_train -> FusedTriplaneTrainHead -> composite_rays_train_triplane -> objective -> backward, plus the
    jitter regulariser through a second head forward; every parameter gradient against the same step on the torch restatement"""
    from conftest import ellipsoid_bitfield, synthetic_camera
    from lzzx_nerf_amd import raymarching as R
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    from lzzx_nerf_amd.objective import HeadObjective, jitter_regularizer
    from oracle.head import get_rays
    H = W = 32
    pose, intr = synthetic_camera(H, W)
    ro, rd = get_rays(pose, intr, H, W)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = dict(record_dtype="f16", forward_dtype="f16", backward_dtype="f16") if arr == "O" else {}
    net = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0, **kw).cuda()
    scale = 2.0 ** 16 if arr == "O" else 1.0
    aabb = dev(np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32))
    nears, fars = R.near_far_from_aabb(dev(ro), dev(rd), aabb, 0.05)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, deltas, rays = R.march_rays_train(dev(ro), dev(rd), 1.0, dev(ellipsoid_bitfield()[0]), 1, 128, nears, fars, ctr, -1, True, 128,
                                                  True, 1 / 256, 16)
    xyzs, dirs = xyzs.contiguous(), dirs.contiguous()
    enc_a, ind, eye = dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"])
    N = H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    target = torch.rand(N, 3, device="cuda", generator=g)
    face = torch.rand(N, device="cuda", generator=g) < 0.4
    bg = torch.rand(N, 3, device="cuda", generator=g)
    delta = (torch.rand(xyzs.shape, device="cuda", generator=g) * 2 - 1) * 1e-3
    step, obj = 96000, HeadObjective(200000)
    sf = obj.step_factor(step)

    def run(fused):
        net.zero_grad(set_to_none=True)
        sigma, rgb, a0, a1, unc = net(xyzs, dirs, enc_a, ind, eye)
        ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sigma, rgb, a0.squeeze(-1), a1.squeeze(-1), unc.squeeze(-1), deltas, rays)
        with torch.no_grad():
            _, _, r0, r1, r2 = net(xyzs, dirs, enc_a, ind, eye)
        _, _, j0, j1, j2 = net(xyzs + delta, dirs, enc_a, ind, eye)
        if fused:
            loss, _, _ = obj(img, ws, a0s, a1s, us, bg, target, face, step)
            loss = loss + jitter_regularizer((r2, r0, r1), (j2, j0, j1), sf, obj.regularizer_flags())
        else:
            loss, _, _ = S.head_objective(img, ws, a0s, a1s, us, bg, target, face, sf, (True, True, True))
            loss = loss + S.jitter((r2, r0, r1), (j2, j0, j1), sf, (True, True, True))
        (loss * scale).backward()
        return float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    lf, gf = run(True)
    lt, gt = run(False)
    assert lf == pytest.approx(lt, rel=1e-5)
    assert set(gf) == set(gt) and len(gf) > 0
    for k in gt:
        a, b = gf[k].double().cpu().numpy(), gt[k].double().cpu().numpy()
        scale = max(np.abs(b).max(), 1e-12)
        assert np.max(np.abs(a - b)) / scale < 2e-3, (k, np.max(np.abs(a - b)) / scale)
