"""LPIPS v0.1 on the AlexNet trunk, the definition of DESIGN 4.14 restated in torch on the CPU with F.conv2d and F.max_pool2d, for any
dtype: float64 it is what the kernels of csrc/lz_lpips.hip are held to (tests/test_gpu_lpips.py), float32 it measures how far an f32
evaluation of the same definition lands from it (tests/lpips_cases.py).  The gradient comes from torch autograd.  `plain_value` is a
second evaluation with Python loops, which test_lpips_host.py holds this one to."""
import numpy as np
import torch
import torch.nn.functional as F

CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
STRIDE_PAD = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))
POOL_BEFORE = (False, True, True, False, False)     # maxpool 3 / 2 in front of conv2 and conv3
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10


def weights(state, dtype):
    """the state dict (numpy arrays or tensors) -> dict of CPU tensors of `dtype`: conv_w, conv_b, lin [C], shift / scale [1,3,1,1]"""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    w = {"conv_w": [t(state[k + ".weight"]) for k in CONV_KEYS], "conv_b": [t(state[k + ".bias"]) for k in CONV_KEYS],
         "lin": [t(state[f"lin{i}.model.1.weight"]).reshape(-1) for i in range(5)]}
    w["shift"] = t(state.get("scaling_layer.shift", np.array(SHIFT, np.float32))).reshape(1, 3, 1, 1)
    w["scale"] = t(state.get("scaling_layer.scale", np.array(SCALE, np.float32))).reshape(1, 3, 1, 1)
    return w


def features(w, x):
    """the five taps (after every ReLU) of images x [P,3,H,W]"""
    h = (x - w["shift"]) / w["scale"]
    taps = []
    for i in range(5):
        if POOL_BEFORE[i]:
            h = F.max_pool2d(h, 3, 2)
        h = F.relu(F.conv2d(h, w["conv_w"][i], w["conv_b"][i], stride=STRIDE_PAD[i][0], padding=STRIDE_PAD[i][1]))
        taps.append(h)
    return taps


def tap_distances(w, pred, target):
    """[5, P]: per tap, the spatial mean of sum_c lin_c (n_pred - n_target)^2"""
    out = []
    for i, (a, b) in enumerate(zip(features(w, pred), features(w, target))):
        na = a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + EPS)
        nb = b / (torch.sqrt((b ** 2).sum(1, keepdim=True)) + EPS)
        out.append((w["lin"][i].reshape(1, -1, 1, 1) * (na - nb) ** 2).sum(1).mean((1, 2)))
    return torch.stack(out)


def lpips(w, pred, target):
    """[P]"""
    return tap_distances(w, pred, target).sum(0)


def value_and_grad(state, pred, target, dtype, upstream=None):
    """pred / target: numpy [P,3,H,W] -> (value [P], d (sum_p upstream[p] value[p]) / d pred) as numpy arrays of `dtype`"""
    w = weights(state, dtype)
    a = torch.as_tensor(pred).to(dtype).requires_grad_(True)
    b = torch.as_tensor(target).to(dtype)
    v = lpips(w, a, b)
    u = torch.ones_like(v) if upstream is None else torch.as_tensor(upstream).to(dtype)
    (v * u).sum().backward()
    return v.detach().numpy(), a.grad.numpy()


def plain_value(state, pred, target):
    """LPIPS of ONE pair of [3,H,W] images in float64 by plain loops over numpy scalars and rows (no conv2d, no max_pool2d): slow, for the
    smallest shape only"""
    sd = {k: np.asarray(v, np.float64) for k, v in state.items()}
    shift = sd.get("scaling_layer.shift", np.array(SHIFT, np.float64)).reshape(3)
    scale = sd.get("scaling_layer.scale", np.array(SCALE, np.float64)).reshape(3)

    def conv(x, W, b, stride, pad):
        C, H, Wd = x.shape
        K = W.shape[2]
        xp = np.zeros((C, H + 2 * pad, Wd + 2 * pad))
        xp[:, pad:pad + H, pad:pad + Wd] = x
        Ho, Wo = (H + 2 * pad - K) // stride + 1, (Wd + 2 * pad - K) // stride + 1
        out = np.zeros((W.shape[0], Ho, Wo))
        for oy in range(Ho):
            for ox in range(Wo):
                win = xp[:, oy * stride:oy * stride + K, ox * stride:ox * stride + K]
                for co in range(W.shape[0]):
                    out[co, oy, ox] = max((win * W[co]).sum() + b[co], 0.0)
        return out

    def pool(x):
        C, H, Wd = x.shape
        Ho, Wo = (H - 3) // 2 + 1, (Wd - 3) // 2 + 1
        out = np.zeros((C, Ho, Wo))
        for oy in range(Ho):
            for ox in range(Wo):
                out[:, oy, ox] = x[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].reshape(C, -1).max(1)
        return out

    def taps(img):
        h = (np.asarray(img, np.float64) - shift[:, None, None]) / scale[:, None, None]
        out = []
        for i, k in enumerate(CONV_KEYS):
            if POOL_BEFORE[i]:
                h = pool(h)
            h = conv(h, sd[k + ".weight"], sd[k + ".bias"], *STRIDE_PAD[i])
            out.append(h)
        return out

    total = 0.0
    for i, (a, b) in enumerate(zip(taps(pred), taps(target))):
        lin = sd[f"lin{i}.model.1.weight"].reshape(-1)
        C, H, Wd = a.shape
        s = 0.0
        for y in range(H):
            for x in range(Wd):
                na = a[:, y, x] / (np.sqrt((a[:, y, x] ** 2).sum()) + EPS)
                nb = b[:, y, x] / (np.sqrt((b[:, y, x] ** 2).sum()) + EPS)
                s += float((lin * (na - nb) ** 2).sum())
        total += s / (H * Wd)
    return total
