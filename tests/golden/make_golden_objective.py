#!/usr/bin/env python3
"""Generate tests/golden/reference_objective.npz by RUNNING the reference's own, unmodified TrainerUtil.train_step
(/root/reference/nerf_triplane/TrainerUtil.py:187-367) on the CPU (build container only; nothing at test time imports the reference).

train_step is called on `object.__new__(TrainerUtil)` with a SimpleNamespace `opt`, criterion = MSELoss(reduction='none') (train.py:207)
and a stub model:
  * model.render / render_torso return LEAF tensors (image_raw, weights_sum, ambient sums, uncertainty; torso_color), the head image
    blended and clamped as renderer.py:380-382 does, plus the `rays` tuple the regulariser reads;
  * model.__call__ is a tiny deterministic function of the sample positions (one 3x3 parameter), called by the regulariser at xyzs
    (no grad) and at xyzs + xyz_delta; torch's CPU RNG is seeded before each call, so the reference draws a reproducible xyz_delta.
global_step is incremented before train_step as the trainer does (TrainerUtil.py:861).  The inputs are an integer hash of (case seed,
element index) (tests/objective_spec.py: case_inputs), so the fixture stores only how to rebuild them; after loss.backward() it stores
the reference's loss, the gradients of the leaves and the regulariser's two forwards with the gradient of the jittered one.  `terms` are NOT the reference's
(its loss is one accumulated tensor): they are tests/objective_spec.py in float32 on the same inputs, and the script asserts that they
add up to the reference's loss.  Third-party modules train_step never touches are empty stubs.

Run:  python tests/golden/make_golden_objective.py
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, TESTS)

import objective_spec as S  # noqa: E402


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return type(k, (), {})


for _n in ("cv2", "imageio", "tensorboardX", "trimesh", "pydub", "torch_ema", "lpips", "mcubes", "dlib", "face_alignment", "numba"):
    sys.modules[_n] = _Stub(_n)

from nerf_triplane.TrainerUtil import TrainerUtil  # noqa: E402  (reference)

ITERS = 200000      # train.py:28


class StubModel:
    def __init__(self, leaves, M, seed):
        self.leaves = leaves
        g = torch.Generator().manual_seed(seed)
        self.W = torch.nn.Parameter(torch.randn(3, 3, generator=g))
        self.xyzs = torch.rand(M, 3, generator=g) * 2 - 1
        self.calls = []
        self.anchor_points = leaves.get("anchor_points")

    def render(self, rays_o, rays_d, auds, bg_coords, poses, eye=None, index=None, staged=False, bg_color=None, perturb=True,
               force_all_rays=False, **kw):
        L = self.leaves
        image = L["image_raw"] + (1 - L["ws"]).unsqueeze(-1) * bg_color        # renderer.py:380-382
        image = image.view(1, -1, 3).clamp(0, 1)
        M = self.xyzs.shape[0]
        rays = (self.xyzs, torch.zeros(M, 3), torch.zeros(1, 32), torch.zeros(1, 4), torch.zeros(1, 1))
        return dict(image=image, weights_sum=L["ws"], ambient_aud=L["aud"].view(1, -1), ambient_eye=L["eye"].view(1, -1),
                    uncertainty=L["unc"], rays=rays)

    def render_torso(self, rays_o, rays_d, auds, bg_coords, poses, **kw):
        return dict(torso_color=self.leaves["torso_color"].view(1, -1, 3))

    def __call__(self, xyzs, dirs, enc_a, ind_code, eye):
        h = xyzs @ self.W
        unc = torch.nn.functional.softplus(5 * h[:, 0:1])
        aud = torch.sigmoid(7 * h[:, 1:2])
        eye_ = torch.tanh(3 * h[:, 2:3])
        out = (torch.zeros_like(unc), torch.zeros_like(xyzs), aud, eye_, unc)
        if torch.is_grad_enabled():
            for t in out[2:]:
                t.retain_grad()
        self.calls.append(out)
        return out


def make_inputs(N, seed, face, bg, image_lo, image_hi):
    x = S.case_inputs(N, seed, face, bg, image_lo, image_hi)       # hashed from (seed, index): the fixture does not store them
    return {k: torch.from_numpy(np.asarray(v)) for k, v in x.items()}


def run_head(name, N, step, iters=ITERS, flags=(True, True, True), face="mixed", bg="scalar", image_lo=-0.125, image_hi=1.125, M=256, seed=0):
    x = make_inputs(N, seed, face, bg, image_lo, image_hi)
    leaves = {k: x[k].clone().requires_grad_(True) for k in ("image_raw", "ws", "aud", "eye", "unc")}
    model = StubModel(leaves, M, seed + 1)
    opt = SimpleNamespace(torso=False, color_space="srgb", patch_size=1, train_camera=False, finetune_lips=False, iters=iters,
                          unc_loss=flags[0], amb_aud_loss=flags[1], amb_eye_loss=flags[2], lambda_amb=1e-4, max_steps=16)
    t = object.__new__(TrainerUtil)
    t.opt, t.criterion, t.log_ptr, t.model, t.flip_finetune_lips = opt, torch.nn.MSELoss(reduction="none"), None, model, False
    t.global_step = step - 1
    t.global_step += 1                                                      # TrainerUtil.py:861
    bg_arg = x["bg"] if x["bg"].dim() else float(x["bg"])
    data = dict(rays_o=torch.zeros(1, N, 3), rays_d=torch.zeros(1, N, 3), bg_coords=torch.zeros(1, N, 2), poses=torch.eye(4)[None],
                face_mask=x["face"].view(1, N), eye_mask=None, lhalf_mask=None, eye=torch.zeros(1, 1), auds=torch.zeros(1, 29, 16),
                index=torch.zeros(1, dtype=torch.long), images=x["target"].view(1, N, 3), bg_color=bg_arg)
    torch.manual_seed(1234 + seed)                                          # the regulariser's torch.rand
    _, _, loss = t.train_step(data)
    loss.backward()
    sf = min(step / iters, 1.0)
    with torch.no_grad():
        l32, _, terms = S.head_objective(x["image_raw"], x["ws"], x["aud"], x["eye"], x["unc"], bg_arg, x["target"], x["face"], sf, flags)
    out = {"N": np.int64(N), "seed": np.int64(seed), "face_mode": np.array(face), "bg_mode": np.array(bg), "image_lo": np.float64(image_lo),
           "image_hi": np.float64(image_hi), "step": np.int64(step), "iters": np.int64(iters), "flags": np.array(flags, dtype=np.bool_),
           "loss": np.float32(loss.item()), "terms": np.array([float(terms[k]) for k in S.TERMS], np.float32)}
    for k, v in leaves.items():
        if v.grad is not None:                                           # an input the objective does not read gets none
            out["g_" + k] = v.grad.numpy()
    reg = step % 16 == 0
    out["regularized"] = np.bool_(reg)
    if reg:
        assert len(model.calls) == 2
        raw, jit = model.calls
        for j, k in enumerate(("unc", "aud", "eye")):
            i = {"unc": 4, "aud": 2, "eye": 3}[k]
            out["raw_" + k] = raw[i].detach().numpy()
            out["reg_" + k] = jit[i].detach().numpy()
            if jit[i].grad is not None:
                out["g_reg_" + k] = jit[i].grad.numpy()
        with torch.no_grad():
            rl = S.jitter([raw[4], raw[2], raw[3]], [jit[4], jit[2], jit[3]], sf, flags)
        out["reg_loss"] = np.float32(float(rl))
        l32 = l32 + rl
    err = abs(float(l32) - loss.item())
    assert err <= 2e-6 * max(1.0, abs(loss.item())), (name, float(l32), loss.item())
    return {name + "__" + k: v for k, v in out.items()}


def run_torso(name, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = S.torso_inputs(N, seed)
    color = torch.from_numpy(x["torso_color"]).requires_grad_(True)
    target = torch.from_numpy(x["target"])
    anchors = torch.nn.Parameter(torch.tensor([[0.01, 0.01, 0.1, 1], [-0.1, -0.1, 0.1, 1], [0.1, -0.1, 0.1, 1]]) + 0.05 * torch.randn(3, 4, generator=g))
    model = StubModel({"torso_color": color, "anchor_points": anchors}, 1, seed)
    opt = SimpleNamespace(torso=True, color_space="srgb", patch_size=1, train_camera=False, finetune_lips=False, iters=ITERS,
                          unc_loss=True, amb_aud_loss=True, amb_eye_loss=True, lambda_amb=1e-4, max_steps=16)
    t = object.__new__(TrainerUtil)
    t.opt, t.criterion, t.log_ptr, t.model, t.flip_finetune_lips = opt, torch.nn.MSELoss(reduction="none"), None, model, False
    t.global_step = 16                                                      # a regulariser step: the torso path returns before it
    data = dict(rays_o=torch.zeros(1, N, 3), rays_d=torch.zeros(1, N, 3), bg_coords=torch.zeros(1, N, 2), poses=torch.eye(4)[None],
                face_mask=torch.zeros(1, N, dtype=torch.bool), eye_mask=None, lhalf_mask=None, eye=torch.zeros(1, 1),
                auds=torch.zeros(1, 29, 16), index=torch.zeros(1, dtype=torch.long), bg_torso_color=target.view(1, N, 3), bg_color=1.0)
    _, _, loss = t.train_step(data)
    loss.backward()
    out = {"N": np.int64(N), "seed": np.int64(seed), "anchor_points": anchors.detach().numpy(),
           "loss": np.float32(loss.item()), "g_torso_color": color.grad.numpy(), "g_anchor_points": anchors.grad.numpy()}
    return {name + "__" + k: v for k, v in out.items()}


CASES = [
    dict(name="step1", N=256, step=1),
    dict(name="step300", N=256, step=300, bg="ray"),
    dict(name="step_iters", N=1000, step=ITERS, bg="ray"),
    dict(name="step_2iters", N=256, step=2 * ITERS),
    dict(name="step_mult16", N=256, step=96000, bg="zero"),
    dict(name="mid", N=256, step=600, iters=1000),
    dict(name="no_unc", N=256, step=96000, flags=(False, True, True)),
    dict(name="no_amb_eye", N=256, step=96016, flags=(True, True, False)),
    dict(name="no_amb_aud", N=256, step=600, iters=1000, flags=(True, False, False)),
    dict(name="no_flags", N=256, step=96000, flags=(False, False, False)),
    dict(name="face_all", N=256, step=600, iters=1000, face="all", bg="ray"),
    dict(name="face_none", N=256, step=600, iters=1000, face="none"),
    dict(name="clamp_heavy", N=256, step=600, iters=1000, bg="ray", image_lo=-1.0, image_hi=2.0),
    dict(name="n1", N=1, step=600, iters=1000),
    dict(name="n4097", N=4097, step=ITERS, bg="ray", M=1024),
]


def main():
    out = {}
    for c in CASES:
        c = dict(c)
        name = c.pop("name")
        out.update(run_head(name, **c))
    out.update(run_torso("torso", 256))
    out["head_cases"] = np.array([c["name"] for c in CASES])
    path = os.path.join(HERE, "reference_objective.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays")


if __name__ == "__main__":
    main()
