"""The reference's training objective (TrainerUtil.train_step, /root/reference/nerf_triplane/TrainerUtil.py:233-367) on the kernels of
csrc/lz_objective.hip, as autograd Functions:

    HeadObjective(iters, ...)(image_raw, weights_sum, amb_aud_sum, amb_eye_sum, uncertainty_sum, bg_color, target, face_mask, global_step)
        -> (loss, pred_rgb, terms)     pred_rgb = clamp(image_raw + (1 - weights_sum) bg, 0, 1) (renderer.py:380-382); terms [6] =
                                       (mse, unc_nll, unc_static, entropy, amb_aud, amb_eye), each as it enters the loss
    TorsoObjective()(torso_color, target, anchor_points) -> (loss, terms [2])
    jitter_regularizer(raw, reg, step_factor, flags) -> loss   (:346-365; add it to the head loss when global_step % 16 == 0)

The head objective is two launches forward (one without unc_loss) and one backward; each of the others one and one.  No host
synchronisation: the upstream gradient (1, or a GradScaler's scale) is read on the device.  All inputs are f32 (under autocast they are
cast to f32, as the reference's are: every input of its objective is f32).

The two LPIPS branches of train_step (:274-284 for patch_size > 1, :291-309 for finetune_lips) run when HeadObjective is given a
perceptual.FusedLPIPS (`lpips=`): the term is computed on pred_rgb, in f32 (the reference runs it under autocast), and its gradient
reaches image_raw and weights_sum through the clamp by lz_objective_pred_backward; `terms` then has a seventh element, the LPIPS term as
it enters the loss.  Without `lpips` both options are rejected, as before.  Out of scope, as in the rest of the package: color_space
'linear' (convert the target first) and the LPIPS / LMD meters."""
import torch
from torch.autograd import Function

from ._lib import LZ_OBJ_AMB_AUD, LZ_OBJ_AMB_EYE, LZ_OBJ_UNC, LZ_OBJECTIVE_WS_BYTES
from ._util import call, ptr, stream, workspace

def _workspace(device):
    """LZ_OBJECTIVE_WS_BYTES per device, zeroed once (the kernels leave their tickets at 0); launches on it are ordered by the stream"""
    return workspace("objective", device, LZ_OBJECTIVE_WS_BYTES, zero=True)


def _rays(t, name, n_last, dtype=torch.float32):
    """[N, n_last] / [1, N, n_last] (n_last None: [N] / [1, N]) -> contiguous [N(, n_last)] of `dtype`; B > 1 is rejected"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    shape = tuple(t.shape)
    want = 1 if n_last is None else 2
    if len(shape) == want + 1:
        if shape[0] != 1:
            raise ValueError(f"{name}: batch size {shape[0]} (only B == 1 is supported, as the reference's trainer)")
        t = t[0]
    elif len(shape) != want:
        raise ValueError(f"{name}: shape {shape}")
    if n_last is not None and t.shape[-1] != n_last:
        raise ValueError(f"{name}: shape {shape}, last dimension must be {n_last}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor")
    return t.to(dtype).contiguous()


def _bg(bg, N, device):
    """(bg_mode, bg_scalar, tensor or None) of include/lzzx_nerf_hip.h: a Python number, a one-element tensor, [3] or [N,3] / [1,N,3]"""
    if not isinstance(bg, torch.Tensor):
        return 0, float(bg), None
    b = bg.to(device=device, dtype=torch.float32)
    if b.numel() == 1:
        return 1, 1.0, b.reshape(1).contiguous()
    if b.numel() == 3:
        return 2, 1.0, b.reshape(3).contiguous()
    if b.numel() == N * 3 and b.shape[-1] == 3:
        return 3, 1.0, b.reshape(N, 3).contiguous()
    raise ValueError(f"bg_color: shape {tuple(bg.shape)} (a number, [1], [3] or [N,3])")


class _HeadObjective(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, image, ws, aud, eye, unc, target, face, bg_mode, bg_scalar, bg, flags, sf, lambda_amb, max_steps):
        N = ws.shape[0]
        dev = ws.device
        pred = torch.empty(N, 3, device=dev)
        loss = torch.empty((), device=dev)
        aux = torch.empty(8, device=dev)
        call("lz_objective_head_forward", ptr(image), ptr(ws), ptr(bg), bg_mode, bg_scalar, ptr(target), ptr(face), ptr(unc), ptr(aud), ptr(eye), N,
             flags, sf, lambda_amb, max_steps, ptr(pred), ptr(loss), ptr(aux), ptr(_workspace(dev)), stream())
        ctx.save_for_backward(image, ws, aud, eye, unc, target, face, bg, aux)
        ctx.args = (bg_mode, bg_scalar, flags, sf, lambda_amb, max_steps)
        terms = aux[:6]
        ctx.mark_non_differentiable(pred, terms)
        return loss, pred, terms

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_loss, _g_pred, _g_terms):
        image, ws, aud, eye, unc, target, face, bg, aux = ctx.saved_tensors
        bg_mode, bg_scalar, flags, sf, lambda_amb, max_steps = ctx.args
        N = ws.shape[0]
        g = g_loss.float().contiguous()
        g_img, g_ws = torch.empty_like(image), torch.empty_like(ws)
        g_unc = torch.empty_like(ws) if flags & LZ_OBJ_UNC else None
        g_aud = torch.empty_like(ws) if flags & LZ_OBJ_AMB_AUD else None
        g_eye = torch.empty_like(ws) if flags & LZ_OBJ_AMB_EYE else None
        call("lz_objective_head_backward", ptr(g), ptr(image), ptr(ws), ptr(bg), bg_mode, bg_scalar, ptr(target), ptr(face), ptr(unc), ptr(aud),
             ptr(eye), ptr(aux), N, flags, sf, lambda_amb, max_steps, ptr(g_img), ptr(g_ws), ptr(g_unc), ptr(g_aud), ptr(g_eye), stream())
        return (g_img, g_ws, g_aud, g_eye, g_unc) + (None,) * 9


class _PredRGB(Function):
    """pred_rgb of _HeadObjective made differentiable: the same values, and the gradient back through the clamp and the blend"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pred, image, ws, bg_mode, bg_scalar, bg):
        ctx.save_for_backward(image, ws, bg)
        ctx.args = (bg_mode, bg_scalar)
        return pred.view_as(pred)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_pred):
        image, ws, bg = ctx.saved_tensors
        bg_mode, bg_scalar = ctx.args
        g = g_pred.float().contiguous()
        g_img, g_ws = torch.empty_like(image), torch.empty_like(ws)
        call("lz_objective_pred_backward", ptr(g), ptr(image), ptr(ws), ptr(bg), bg_mode, bg_scalar, ws.shape[0], ptr(g_img), ptr(g_ws), stream())
        return None, g_img, g_ws, None, None, None


LPIPS_PATCH_WEIGHT, LPIPS_LIPS_WEIGHT, LPIPS_LIPS_MIN = 0.1, 0.01, 32      # TrainerUtil.py:284, :309, :298-299


class HeadObjective:
    """TrainerUtil.train_step for the head (opt.torso off, B == 1); defaults of train.py:28,35,48-51.
    amb_eye_loss without amb_aud_loss is rejected: the reference's eye term reads the audio term's lambda and input (a NameError there).

    lpips: a perceptual.FusedLPIPS, needed for patch_size > 1 and finetune_lips (a ValueError without it).  patch_size > 1 adds
    0.1 * mean_p LPIPS over the rays viewed as [-1, ps, ps, 3] (:275-284; N a multiple of ps^2, ps >= 31).  finetune_lips makes __call__
    accept rect=(xmin, xmax, ymin, ymax): on a step that gives it, 0.01 * LPIPS of the view [1, xmax-xmin, ymax-ymin, 3], scaled to
    [-1, 1] and then zero-padded symmetrically to at least 32 (:295-303; N must equal the rectangle's area), is added; with rect=None the
    term is absent and the step is today's objective bit for bit -- the caller alternates, as the reference flips opt.finetune_lips.
    unc_loss=False gives the reference's arrangement while flip_finetune_lips is on."""

    def __init__(self, iters, unc_loss=True, amb_aud_loss=True, amb_eye_loss=True, lambda_amb=1e-4, max_steps=16, patch_size=1,
                 finetune_lips=False, lpips=None):
        if (patch_size > 1 or finetune_lips) and lpips is None:
            raise ValueError("the LPIPS terms (patch_size > 1, finetune_lips) are not implemented without lpips= (a perceptual.FusedLPIPS)")
        if patch_size > 1 and patch_size < 31:
            raise ValueError(f"patch_size {patch_size}: the LPIPS trunk needs patches of at least 31 x 31")
        self.lpips, self.patch_size, self.finetune_lips = lpips, int(patch_size), bool(finetune_lips)
        if amb_eye_loss and not amb_aud_loss:
            raise ValueError("amb_eye_loss needs amb_aud_loss (the reference's eye term uses its lambda and ambient_aud)")
        if iters <= 0:
            raise ValueError(f"iters {iters}")
        self.iters, self.lambda_amb, self.max_steps = iters, float(lambda_amb), float(max_steps)
        self.unc_loss, self.amb_aud_loss, self.amb_eye_loss = bool(unc_loss), bool(amb_aud_loss), bool(amb_eye_loss)
        self.flags = (LZ_OBJ_UNC if unc_loss else 0) | (LZ_OBJ_AMB_AUD if amb_aud_loss else 0) | (LZ_OBJ_AMB_EYE if amb_eye_loss else 0)

    def step_factor(self, global_step):
        return min(global_step / self.iters, 1.0)

    def regularizer_flags(self):
        """the `flags` argument of jitter_regularizer for this configuration"""
        return (self.unc_loss, self.amb_aud_loss, self.amb_eye_loss)

    @staticmethod
    def wants_regularizer(global_step):
        return global_step % 16 == 0

    def __call__(self, image_raw, weights_sum, amb_aud_sum, amb_eye_sum, uncertainty_sum, bg_color, target, face_mask, global_step, rect=None):
        ws = _rays(weights_sum, "weights_sum", None)
        N = ws.shape[0]
        if N == 0:
            raise ValueError("no rays (N = 0)")
        if rect is not None and not self.finetune_lips:
            raise ValueError("rect is the lips rectangle of finetune_lips=True")
        views = []      # (coefficient, image height, image width, pad to 32) of the LPIPS terms of this step
        if self.patch_size > 1:
            ps = self.patch_size
            if N % (ps * ps):
                raise ValueError(f"{N} rays are no multiple of patch_size^2 = {ps * ps}")
            views.append((LPIPS_PATCH_WEIGHT, ps, ps, False))
        if rect is not None:
            xmin, xmax, ymin, ymax = (int(v) for v in rect)
            h, w = xmax - xmin, ymax - ymin
            if h <= 0 or w <= 0 or h * w != N:
                raise ValueError(f"rect {tuple(rect)} holds {max(h, 0)} x {max(w, 0)} rays, N = {N}")
            views.append((LPIPS_LIPS_WEIGHT, h, w, True))
        image = _rays(image_raw, "image_raw", 3)
        tgt = _rays(target, "target", 3)
        if not isinstance(face_mask, torch.Tensor) or face_mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("face_mask must be a bool or uint8 tensor")
        face = _rays(face_mask.view(torch.uint8), "face_mask", None, torch.uint8)
        per_ray = {"unc": (uncertainty_sum, self.unc_loss, "uncertainty_sum"), "aud": (amb_aud_sum, self.amb_aud_loss, "amb_aud_sum"),
                   "eye": (amb_eye_sum, self.amb_eye_loss, "amb_eye_sum")}
        t = {}
        for k, (x, used, name) in per_ray.items():
            t[k] = _rays(x, name, None) if used or x is not None else None      # a missing tensor that is used: ValueError
        for name, x in (("image_raw", image), ("target", tgt), ("face_mask", face)) + tuple((n, t[k]) for k, (_, _, n) in per_ray.items()):
            if x is not None and x.shape[0] != N:
                raise ValueError(f"{name}: {x.shape[0]} rays, weights_sum has {N}")
        bg_mode, bg_scalar, bg = _bg(bg_color, N, ws.device)
        sf = self.step_factor(global_step)
        # the inputs as the caller gave them go to the Function (their gradients flow back through the reshapes above)
        loss, pred, terms = _HeadObjective.apply(_flat(image_raw, 3), _flat(weights_sum, None), _flat_opt(amb_aud_sum), _flat_opt(amb_eye_sum),
                                                 _flat_opt(uncertainty_sum), tgt, face, bg_mode, bg_scalar, bg, self.flags, sf,
                                                 self.lambda_amb, self.max_steps)
        if views:
            # the reference's expressions on pred_rgb and rgb (:275-277, :295-303); the clamp's and the blend's backward is _PredRGB's
            pred_d = _PredRGB.apply(pred, _flat(image_raw, 3), _flat(weights_sum, None), bg_mode, bg_scalar, bg)
            extra = None
            for coef, h, w, pad in views:
                a = pred_d.view(-1, h, w, 3).permute(0, 3, 1, 2).contiguous() * 2 - 1
                b = tgt.detach().view(-1, h, w, 3).permute(0, 3, 1, 2).contiguous() * 2 - 1
                if pad:
                    pad_h, pad_w = max(0, (LPIPS_LIPS_MIN - h + 1) // 2), max(0, (LPIPS_LIPS_MIN - w + 1) // 2)
                    if pad_h or pad_w:
                        a = torch.nn.functional.pad(a, (pad_w, pad_w, pad_h, pad_h))
                        b = torch.nn.functional.pad(b, (pad_w, pad_w, pad_h, pad_h))
                term = coef * self.lpips(a, b).mean()
                extra = term if extra is None else extra + term
            loss = loss + extra
            terms = torch.cat([terms, extra.detach().reshape(1)])
        elif self.lpips is not None:
            terms = torch.cat([terms, terms.new_zeros(1)])
        return loss, pred.view(image_raw.shape), terms


def _flat(t, n_last):
    t = t.reshape(-1) if n_last is None else t.reshape(-1, n_last)
    return t.float().contiguous()


def _flat_opt(t):
    return None if t is None else _flat(t, None)


class _TorsoObjective(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, color, target, anchors):
        N, J = color.shape[0], anchors.shape[0]
        loss = torch.empty((), device=color.device)
        aux = torch.empty(2, device=color.device)
        call("lz_objective_torso_forward", ptr(color), ptr(target), ptr(anchors), J, N, ptr(loss), ptr(aux), ptr(_workspace(color.device)), stream())
        ctx.save_for_backward(color, target, anchors)
        ctx.mark_non_differentiable(aux)
        return loss, aux

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_loss, _g_aux):
        color, target, anchors = ctx.saved_tensors
        g = g_loss.float().contiguous()
        g_color, g_anchors = torch.empty_like(color), torch.empty_like(anchors)
        call("lz_objective_torso_backward", ptr(g), ptr(color), ptr(target), ptr(anchors), anchors.shape[0], color.shape[0], ptr(g_color),
             ptr(g_anchors), stream())
        return g_color, None, g_anchors


class TorsoObjective:
    """TrainerUtil.train_step with opt.torso: the colour MSE plus mean (1 - anchor_points[:, 3])^2.  The reference returns there
    (TrainerUtil.py:244), so its torso-alpha entropy (:319-323) never runs; neither does it here."""

    def __call__(self, torso_color, target, anchor_points):
        color = _rays(torso_color, "torso_color", 3)
        N = color.shape[0]
        if N == 0:
            raise ValueError("no rays (N = 0)")
        tgt = _rays(target, "target", 3)
        if tgt.shape[0] != N:
            raise ValueError(f"target: {tgt.shape[0]} rays, torso_color has {N}")
        if anchor_points.dim() != 2 or anchor_points.shape[1] != 4 or anchor_points.shape[0] == 0:
            raise ValueError(f"anchor_points: shape {tuple(anchor_points.shape)}, want [J,4]")
        loss, terms = _TorsoObjective.apply(_flat(torso_color, 3), tgt, anchor_points.contiguous())
        return loss, terms


class _Jitter(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, flags, scale, raw0, raw1, raw2, reg0, reg1, reg2):
        raws, regs = (raw0, raw1, raw2), (reg0, reg1, reg2)
        M = next(r.shape[0] for r in regs if r is not None)
        dev = next(r.device for r in regs if r is not None)
        loss = torch.empty((), device=dev)
        aux = torch.empty(3, device=dev)
        call("lz_objective_jitter_forward", *[ptr(r) for r in raws], *[ptr(r) for r in regs], M, flags, scale, ptr(loss), ptr(aux),
             ptr(_workspace(dev)), stream())
        ctx.save_for_backward(*raws, *regs)
        ctx.flags, ctx.scale, ctx.M = flags, scale, M
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_loss):
        t = ctx.saved_tensors
        raws, regs = t[:3], t[3:]
        g = g_loss.float().contiguous()
        gr = [torch.empty_like(regs[k]) if ctx.flags & (1 << k) else None for k in range(3)]
        call("lz_objective_jitter_backward", ptr(g), *[ptr(r) for r in raws], *[ptr(r) for r in regs], ctx.M, ctx.flags, ctx.scale,
             *[ptr(x) for x in gr], stream())
        return (None, None, None, None, None) + tuple(gr)


def jitter_regularizer(raw, reg, step_factor, flags):
    """step_factor * 1e-5 * sum over the enabled of (unc, amb_aud, amb_eye) of mean((raw - reg)^2) (TrainerUtil.py:346-365).  raw / reg:
    the (unc, amb_aud, amb_eye) per-sample outputs of the head at xyzs (no grad) and at the jittered xyzs, [M] or [M,1] each; flags: three
    bools (HeadObjective.regularizer_flags()).  The gradient flows into `reg` only, as in the reference."""
    if len(raw) != 3 or len(reg) != 3 or len(flags) != 3:
        raise ValueError("raw, reg and flags are (unc, amb_aud, amb_eye) triples")
    f = sum(1 << k for k in range(3) if flags[k])
    if f == 0:              # the reference adds reg_loss = 0 then
        return torch.zeros((), device=reg[0].device)
    ra, rg = [None] * 3, [None] * 3
    M = None
    for k in range(3):
        if not flags[k]:
            continue
        a, b = raw[k], reg[k]
        if a.shape != b.shape or a.dim() not in (1, 2) or (a.dim() == 2 and a.shape[1] != 1):
            raise ValueError(f"output {k}: raw {tuple(a.shape)} vs reg {tuple(b.shape)} (want equal [M] or [M,1])")
        if M is None:
            M = a.shape[0]
        if a.shape[0] != M:
            raise ValueError(f"output {k}: {a.shape[0]} samples, expected {M}")
        if not (a.is_cuda and b.is_cuda):
            raise ValueError("raw / reg must be CUDA tensors")
        ra[k], rg[k] = a.detach().reshape(-1).float().contiguous(), b.reshape(-1).float().contiguous()
    if M == 0:
        raise ValueError("no samples (M = 0)")
    return _Jitter.apply(f, float(step_factor * 1e-5), *ra, *rg)
