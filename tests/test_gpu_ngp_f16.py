"""BASELINE cfg2 in the reference's autocast arithmetic on the GPU (lzzx_nerf_amd/ngp.py precision="f16", csrc/lz_ngp.hip:
lz_k_ngp_head16): the f16 head against the CPU checker (tests/ngp_fp16_checker.py) on identical half features, against the reference's
own autocast run (tests/golden/reference_ngp_autocast.npz), against torch's CUDA autocast on this project's operators, and the f16
device loop against the reference's host loop around the same head.

The f32 accumulation inside an MFMA runs in the hardware's order, so a half output may round the other way where the exact sum sits near
a rounding boundary: the bound is "at least 90 % of the halves bit-equal, every one within 2 half ulps" (for sigma's pre-activation,
recovered as log(sigma), 2 ulps of the value or of 0.5, whichever is larger: see assert_close)."""
import types

import numpy as np
import pytest
import torch

import ngp_fp16_checker as K
from conftest import ellipsoid_bitfield, synthetic_camera
from oracle import oracle as O

pytestmark = pytest.mark.gpu
F16, F32 = np.float16, np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make(seed=3, precision="f16"):
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    g = GenericHashgridNeRF(torch.device("cuda"), seed=seed)
    fused = FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, precision=precision)
    W = {n: m.net[i].weight.detach().cpu().numpy() for n, m, i in (("sigma_net.net.0", g.sigma_net, 0), ("sigma_net.net.1", g.sigma_net, 1),
                                                                    ("color_net.net.0", g.color_net, 0), ("color_net.net.1", g.color_net, 1))}
    return g, fused, W


def inputs(M, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, (M, 3)).astype(F32)
    d = rng.normal(size=(M, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return x, d


def untile(feats, M):
    """[tile][level][sample][C] (lz_grid_encode_forward_tiled) -> [M, 32]"""
    flat, rows = feats.reshape(-1), []
    for b0 in range(0, M, 256):
        n = min(256, M - b0)
        rows.append(flat[b0 * 32: (b0 + n) * 32].reshape(16, n, 2).permute(1, 0, 2).reshape(n, 32))
    return torch.cat(rows)


def assert_close(sig, rgb, sig_want, rgb_want, pre_want):
    """sig / rgb: the kernel's f32 outputs; sig_want f32, rgb_want / pre_want half"""
    sig, rgb = sig.cpu().numpy(), rgb.cpu().numpy()
    rgb16 = rgb.astype(F16)
    assert np.array_equal(rgb16.astype(F32), rgb)                      # rgb holds halves
    u = K.half_ulps(rgb16, rgb_want)
    assert u.max() <= 2 and (u == 0).mean() >= 0.9, (int(u.max()), float((u == 0).mean()))
    assert (sig == sig_want).mean() >= 0.9, float((sig == sig_want).mean())
    # the half pre-activation recovered, within 2 half ulps -- of the value, or of 0.5 where the value is smaller: near zero one ulp is a
    # tiny absolute step, and a single upstream half rounding that the MFMA order flips (one ulp of a ~1 hidden value in sigma_net.0)
    # moves the pre-activation by up to ~5e-4 whatever its size (the CPU checker against itself with f64 accumulation: 651 ulps at 1.8e-4)
    pre = np.log(sig.astype(np.float64)).astype(F16)
    err = np.abs(pre.astype(F32) - pre_want.astype(F32))
    ulp = np.maximum(np.spacing(np.abs(pre_want.astype(F16))), np.spacing(F16(0.5))).astype(F32)
    assert (err <= 2 * ulp).all(), float((err / ulp).max())
    assert (K.half_ulps(pre, pre_want) == 0).mean() >= 0.9


def head_f16(fused, feats, d, M, count=None):
    from lzzx_nerf_amd._util import call, ptr, stream
    sig, rgb = torch.full((M,), -7.0, device="cuda"), torch.full((M, 3), -7.0, device="cuda")
    call("lz_ngp_head_forward_f16", ptr(fused.packed16), ptr(feats), 2, ptr(d), M, ptr(count), ptr(sig), ptr(rgb), stream())
    torch.cuda.synchronize()
    return sig, rgb


@pytest.mark.parametrize("M", [1, 31, 33, 1000, 70001])
def test_f16_head_against_the_checker(M):
    """the stand-alone head on the f16 gather's own tiled features; the checker on the same features"""
    g, fused, W = make()
    x, d = inputs(M, M + 5, -1.1, 1.1)
    feats = torch.empty(M, 32, dtype=torch.float16, device="cuda")
    fused.encode_tiled(dev(x), feats, 1.0)
    sig, rgb = head_f16(fused, feats, dev(d), M)
    tr = {}
    sig_c, rgb_c = K.head(W, untile(feats, M).cpu().numpy(), d, tr)
    assert_close(sig, rgb, sig_c, rgb_c, tr["sigma_net.net.1"][:, 0])
    # forward() is the same two launches
    s2, r2 = fused.forward(dev(x), dev(d), 1.0)
    assert torch.equal(s2, sig) and torch.equal(r2, rgb)


def test_f16_head_against_the_reference_fixture():
    """weights from the fixture, the table from its recipe: the reference's modules under autocast (exp the CUDA way)"""
    import os
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_ngp_autocast.npz"))
    g = GenericHashgridNeRF(torch.device("cuda"), seed=int(G["table_seed"]))
    e = g.enc.embeddings.detach()
    assert float(e.double().sum()) == float(G["table_sum_f64"])
    mlp = lambda a, b: types.SimpleNamespace(net=[types.SimpleNamespace(weight=dev(G["w/" + a])), types.SimpleNamespace(weight=dev(G["w/" + b]))])
    fused = FusedHashgridNeRF(g.enc, mlp("sigma_net.net.0", "sigma_net.net.1"), mlp("color_net.net.0", "color_net.net.1"), precision="f16")
    sig, rgb = fused.forward(dev(G["xyz"]), dev(G["dirs"]), float(G["bound"]))
    pre = G["lin/sigma_net.net.1"][:, 0]
    assert_close(sig, rgb, O.unary("exp", pre.astype(F32)), G["rgb"], pre)


def test_f16_head_against_torch_cuda_autocast():
    """the drop-in caller's arithmetic: this project's GridEncoder + SHEncoder + nn.Linear(bias=False) under torch.autocast("cuda")"""
    from lzzx_nerf_amd.encoding import get_encoder
    g, fused, W = make()
    sh = get_encoder("spherical_harmonics")[0]
    lin = {}
    for n, w in W.items():
        lin[n] = torch.nn.Linear(w.shape[1], w.shape[0], bias=False).cuda()
        with torch.no_grad():
            lin[n].weight.copy_(dev(w))
    M = 20000
    x, d = inputs(M, 17, -1.1, 1.1)
    tx, td = dev(x), dev(d)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        feat = g.enc(tx, bound=1.0)
        h = lin["sigma_net.net.1"](torch.relu(lin["sigma_net.net.0"](feat)))
        sigma = torch.exp(h[:, 0])
        rgb = torch.sigmoid(lin["color_net.net.1"](torch.relu(lin["color_net.net.0"](torch.cat([sh(td), h[:, 1:]], -1)))))
    assert feat.dtype == h.dtype == rgb.dtype == torch.float16 and sigma.dtype == torch.float32
    s, r = fused.forward(tx, td, 1.0)
    assert_close(s, r, sigma.cpu().numpy(), rgb.cpu().numpy(), h[:, 0].cpu().numpy())


def test_f16_head_count_and_empty_launches():
    """rows behind the device-side count keep what they held; rows = 0 is a no-op that reads no pointer"""
    from lzzx_nerf_amd._lib import load
    from lzzx_nerf_amd._util import stream
    g, fused, W = make()
    M = 5000
    x, d = inputs(M, 3)
    feats = torch.empty(M, 32, dtype=torch.float16, device="cuda")
    fused.encode_tiled(dev(x), feats, 1.0)
    full_s, full_r = head_f16(fused, feats, dev(d), M)
    for c in (0, 1, 37, 2048, M + 10):
        cnt = torch.tensor([c], dtype=torch.int32, device="cuda")
        s, r = head_f16(fused, feats, dev(d), M, cnt)
        k = min(c, M)
        assert torch.equal(s[:k], full_s[:k]) and torch.equal(r[:k], full_r[:k]), c
        assert bool((s[k:] == -7.0).all()) and bool((r[k:] == -7.0).all()), c
    assert load().lz_ngp_head_forward_f16(None, None, 2, None, 0, None, None, None, stream()) == 0
    s = torch.full((4,), -7.0, device="cuda")
    assert load().lz_ngp_head_forward_f16(fused.packed16.data_ptr(), feats.data_ptr(), 2, dev(d).data_ptr(), 0, None, s.data_ptr(),
                                          s.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert bool((s == -7.0).all())


@pytest.mark.parametrize("H,max_steps", [(64, 16), (64, 64), (96, 16), (96, 64)])
def test_f16_renderer_equals_the_host_loop(H, max_steps):
    """HashgridRenderer around a precision="f16" net (lz_ngp_loop_run_f16) against the reference's host loop
    (test_gpu_cfg2_render._render: march_rays -> network -> composite_rays -> compaction) with the GPU f16 head as its network, under the
    reference's schedule (1, 8): image, depth, weights_sum and per-ray counts bit for bit (the head's per-sample arithmetic does not depend
    on a sample's row).  And a sanity bound against the f32 frame."""
    from test_gpu_cfg2_render import _Gpu, _render
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF, HashgridRenderer
    from lzzx_nerf_amd.utils import frame_rays
    g, fused, W = make()
    bits = dev(ellipsoid_bitfield()[0])
    aabb = dev(np.array([-1, -1, -1, 1, 1, 1], F32))
    pose, intr = synthetic_camera(H, H)
    ro, rd = frame_rays(dev(pose), intr, H, H)
    r = HashgridRenderer(fused, bits, bound=1.0, aabb=aabb, budget_factor=1, n_step_cap=8)
    got = {k: v.clone() for k, v in r.render(ro, rd, max_steps=max_steps, count_samples=True).items()}

    class Ops(_Gpu):
        def __init__(self):
            pass

        def net(self, xyzs, dirs, bound):
            return fused.forward(xyzs, dirs, bound)
    img, dep, ws, cnt = _render(Ops(), ro, rd, aabb, bits, 1.0, max_steps)
    assert np.array_equal(got["image"].cpu().numpy(), img.astype(F32))
    assert np.array_equal(got["depth"].cpu().numpy(), dep) and np.array_equal(got["weights_sum"].cpu().numpy(), ws)
    assert np.array_equal(got["ray_counts"].cpu().numpy().astype(np.int64), cnt)
    assert int(got["state"][3]) == 1 and float(got["weights_sum"].max()) > 0.5
    # against the f32 frame of the same network: the half rounding of features, weights and activations moves pixels a little.  Measured
    # on MI355X at these four sizes: max |diff| 7.2e-5 .. 8.6e-5, PSNR 99.7-99.8 dB.  Bound: one half ulp at 0.5 (4.9e-4), the rounding step
    # of a sample's colour near this network's mid-grey, which compositing only averages; and 90 dB
    r32 = HashgridRenderer(FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net), bits, bound=1.0, aabb=aabb, budget_factor=1, n_step_cap=8)
    ref = r32.render(ro, rd, max_steps=max_steps)["image"].cpu().numpy()
    err = np.abs(got["image"].cpu().numpy() - ref)
    psnr = -10 * np.log10(max(float((err ** 2).mean()), 1e-20))
    print("f16 vs f32 frame: max |diff| %.3g, PSNR %.1f dB" % (err.max(), psnr))
    assert err.max() <= float(np.spacing(F16(0.5))) and psnr >= 90.0
