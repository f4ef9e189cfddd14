"""The training objective of TrainerUtil.train_step (TrainerUtil.py:233-367) restated in torch, term by term, for any dtype / device:
float64 on the CPU it is the specification the fused kernels (lzzx_nerf_amd/objective.py) are checked against; float32 on the GPU it is
the unfused baseline of tools/objective_bench.py.  Detached exactly where the reference detaches."""
import numpy as np
import torch

TERMS = ("mse", "unc_nll", "unc_static", "entropy", "amb_aud", "amb_eye")


def head_objective(image_raw, ws, aud, eye, unc, bg, target, face, sf, flags, lambda_amb=1e-4, max_steps=16):
    """image_raw / target [N,3], ws / aud / eye / unc [N], bg a number, [3] or [N,3], face [N] bool; flags = (unc, amb_aud, amb_eye)
    -> (loss, pred [N,3], {term: value})"""
    unc_on, aud_on, eye_on = flags
    N = ws.shape[0]
    P = (image_raw + (1 - ws).unsqueeze(-1) * bg).clamp(0, 1)                    # renderer.py:380-382
    diff = P - target
    per_ray = (diff ** 2).mean(-1)                                               # :238
    f = face.bool()
    zero = per_ray.sum() * 0
    terms = {k: zero for k in TERMS}
    if unc_on:                                                                   # :254-272
        w = (torch.softmax(unc, dim=-1) * N).detach()
        per_ray = per_ray * (0.2 + 0.8 * ((1 - sf) + sf * w).clamp(0, 10))
        beta = unc + 1
        nrm = torch.norm(diff, dim=-1).detach()
        terms["unc_nll"] = (sf * ((nrm / (2 * beta ** 2) + torch.log(beta) ** 2 / 2) * f)).mean()
        terms["unc_static"] = (1e-3 * sf * (unc * (~f))).mean()
    terms["mse"] = per_ray.mean()                                                # :315
    A = ws.clamp(1e-5, 1 - 1e-5)                                                 # :326-328
    terms["entropy"] = 1e-4 * (-A * torch.log2(A) - (1 - A) * torch.log2(1 - A)).mean()
    lam = sf * lambda_amb
    if aud_on:                                                                   # :331-336
        terms["amb_aud"] = lam * (aud * (~f)).mean()
    if eye_on:                                                                   # :339-343
        terms["amb_eye"] = lam * ((eye / max_steps) * aud.detach() * f).mean()
    loss = sum(terms[k] for k in TERMS)
    return loss, P, terms


def jitter(raw, reg, sf, flags):
    """:346-365 -- sf * 1e-5 * sum over the enabled k of mean((raw_k - reg_k)^2); raw is detached (the no-grad forward)"""
    out = 0
    for k in range(3):
        if flags[k]:
            out = out + ((raw[k].detach() - reg[k]) ** 2).mean()
    return out * (sf * 1e-5)


def torso_objective(color, target, anchor_points):
    """:238-244 -- the function returns there: no alpha entropy"""
    return ((color - target) ** 2).mean(-1).mean() + ((1 - anchor_points[:, 3]) ** 2).mean()


_M32 = np.uint64(0xFFFFFFFF)


def hash_unit(seed, salt, shape):
    """values k / 256 (k = 0 .. 255), an integer hash of (seed, salt, element index): the fixture's inputs, the same on every machine and
    numpy / torch version, so tests/golden/reference_objective.npz stores only what the reference computed from them"""
    n = int(np.prod(shape))
    x = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64((seed * 0x85EBCA77 + salt * 0xC2B2AE3D) & 0xFFFFFFFF)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & _M32
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & _M32
    x ^= x >> np.uint64(15)
    return ((x >> np.uint64(24)).astype(np.float32) / np.float32(256)).reshape(shape)


def case_inputs(N, seed, face="mixed", bg="scalar", image_lo=-0.125, image_hi=1.125):
    """the head inputs of one fixture case (float32 numpy): image_raw spans [image_lo, image_hi] so the blend clamps; ws holds 0, 1 and a
    value inside the entropy clamp; face 'mixed' / 'all' / 'none'; bg 'scalar' (1), 'zero' or 'ray' ([N,3])"""
    h = lambda salt, *shape: hash_unit(seed, salt, shape)
    x = dict(image_raw=h(1, N, 3) * np.float32(image_hi - image_lo) + np.float32(image_lo), ws=h(2, N), aud=h(3, N) * np.float32(4),
             eye=h(4, N) * np.float32(16), unc=h(5, N) * np.float32(3), target=h(6, N, 3))
    if N >= 4:
        x["ws"][:3] = (0.0, 1.0, 1e-7)
    x["face"] = {"mixed": h(7, N) < 0.4, "all": np.ones(N, np.bool_), "none": np.zeros(N, np.bool_)}[face]
    x["bg"] = {"scalar": np.float32(1.0), "zero": np.float32(0.0), "ray": h(8, N, 3)}[bg]
    return x


def torso_inputs(N, seed):
    return dict(torso_color=hash_unit(seed, 11, (N, 3)), target=hash_unit(seed, 12, (N, 3)))
