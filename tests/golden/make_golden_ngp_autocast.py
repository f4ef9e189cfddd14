#!/usr/bin/env python3
"""Generate tests/golden/reference_ngp_autocast.npz: BASELINE cfg2's hash-grid NeRF (synthetic.GenericHashgridNeRF.net's composition,
synthetic.py:104-114) on the REFERENCE's own modules -- `get_encoder('hashgrid')` (gridencoder.GridEncoder), `get_encoder(
'spherical_harmonics')` (shencoder.SHEncoder) and two `MLP`s (nerf_triplane/network.py:73-94) -- run entirely under torch autocast with
dtype float16, the arithmetic the reference renders in by default (`-O` => --fp16).  Build container only; only arrays travel.

    h = sigma_net(enc(x));  sigma = exp(h[:, 0]);  rgb = sigmoid(color_net(cat([sh(d), h[:, 1:]])))

There is no CUDA device here, so the region is `torch.autocast("cpu", dtype=torch.float16)`, with two differences from the CUDA policy
that the fixture records (`policy_notes`) and that tests/ngp_fp16_checker.py resolves the CUDA way:

    op / query                        CUDA autocast                        this fixture (CPU autocast)
    torch.is_autocast_enabled()       True inside the region               False (it reports the CUDA state only) -> PATCHED to True
      (grid.py:38: half tables)                                            inside the region, so the encoder gathers half features
    torch.exp(h[:, 0])                fp32 list: half -> f32 -> f32        not listed: half in, half out
    nn.Linear                         half list                            half list
    cat([f32, half])                  promote to f32                       promote to f32
    relu / sigmoid                    not listed: run in the input type    not listed

So the fixture stores the half output of every nn.Linear (forward hooks), the encoder's half features, sigma and rgb as the CPU run
returned them, and the aten op trace (op, input dtypes -> output dtype) below the autocast layer.  sigma is compared the CUDA way:
exp in f32 of the half pre-activation `lin/sigma_net.net.1[:, 0]`.

Parameters: lzzx_nerf_amd.synthetic.GenericHashgridNeRF(torch.device("cpu"), seed=3) -- copied into the reference's modules (offsets
and shapes asserted equal).  The 6.1 M x 2 table is not stored: its recipe (the seed, the shape: GenericHashgridNeRF's
torch.rand(shape, generator=manual_seed(seed)) * 2 - 1), a float64 checksum and a few sampled entries are; the four weight matrices are.

Run:  python tests/golden/make_golden_ngp_autocast.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference and the checker on sys.path, installs the back-end adapters)
from make_golden_autocast import OpTrace  # noqa: E402

SEED = 3            # GenericHashgridNeRF's seed
INPUT_SEED = 7
M = 1536            # positions / directions
BOUND = 1.0
N_SAMPLED = 64      # table entries stored for the recipe check


def main():
    MG.install_backends()
    ROOT = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, ROOT)
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF          # this project: the parameters
    g = GenericHashgridNeRF(torch.device("cpu"), seed=SEED)
    from encoding import get_encoder                                   # the reference
    from nerf_triplane.network import MLP
    enc, dim = get_encoder("hashgrid")
    sh, dim_sh = get_encoder("spherical_harmonics")
    assert dim == 32 and dim_sh == 16
    assert torch.equal(enc.offsets.to(torch.int32), g.enc.offsets.cpu().to(torch.int32)), "offsets differ"
    assert tuple(enc.embeddings.shape) == tuple(g.enc.embeddings.shape)
    sigma_net, color_net = MLP(dim, 16, 64, 2), MLP(dim_sh + 15, 3, 64, 2)
    with torch.no_grad():
        enc.embeddings.copy_(g.enc.embeddings.detach())
        for ref, ours in ((sigma_net, g.sigma_net), (color_net, g.color_net)):
            for i in range(2):
                assert tuple(ref.net[i].weight.shape) == tuple(ours.net[i].weight.shape)
                ref.net[i].weight.copy_(ours.net[i].weight.detach())

    rng = np.random.default_rng(INPUT_SEED)
    x = rng.uniform(-1.15 * BOUND, 1.15 * BOUND, (M, 3)).astype(np.float32)     # some outside the bound: zero features
    d = rng.normal(size=(M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tx, td = torch.from_numpy(x), torch.from_numpy(d)

    layer_out = {}
    hooks = []
    for tag, mlp in (("sigma_net", sigma_net), ("color_net", color_net)):
        for i, lin in enumerate(mlp.net):
            hooks.append(lin.register_forward_hook(lambda m, a, o, name="%s.net.%d" % (tag, i): layer_out.__setitem__(name, o.detach().clone())))
    # grid.py:38 asks torch.is_autocast_enabled(), which reports the CUDA state: answer it as a CUDA run would, inside the region only
    orig = torch.is_autocast_enabled
    tr = OpTrace()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16), tr:
        torch.is_autocast_enabled = lambda *a, **k: True if not a and not k else orig(*a, **k)
        try:
            feat = enc(tx, bound=BOUND)
            h = sigma_net(feat)
            sigma = torch.exp(h[:, 0])
            rgb = torch.sigmoid(color_net(torch.cat([sh(td), h[:, 1:]], -1)))
        finally:
            torch.is_autocast_enabled = orig
    for hk in hooks:
        hk.remove()
    assert feat.dtype == torch.float16 and h.dtype == torch.float16 and rgb.dtype == torch.float16

    emb = g.enc.embeddings.detach().numpy()
    srng = np.random.default_rng(5)
    idx = srng.integers(0, emb.shape[0], N_SAMPLED)
    out = dict(
        table_seed=np.array(SEED), table_shape=np.array(emb.shape), table_sum_f64=np.array(emb.astype(np.float64).sum()),
        table_abssum_f64=np.array(np.abs(emb.astype(np.float64)).sum()), table_idx=idx, table_rows=emb[idx],
        offsets=g.enc.offsets.cpu().numpy().astype(np.int32), per_level_scale=np.array(g.enc.per_level_scale, np.float64),
        bound=np.array(BOUND, np.float32), xyz=x, dirs=d, feats=feat.numpy(), sigma=sigma.numpy(), rgb=rgb.numpy(),
        op_trace=np.array(tr.rows), autocast_query_patched=np.array(True),
        policy_notes=np.array(["torch.is_autocast_enabled() patched to True inside the region (grid.py:38 reports the CUDA state only)",
                               "exp: CPU autocast half -> half (recorded sigma); CUDA: fp32 list, half -> f32 (the checker's sigma)"]),
    )
    for tag, mlp in (("sigma_net", sigma_net), ("color_net", color_net)):
        for i in range(2):
            name = "%s.net.%d" % (tag, i)
            out["w/" + name] = mlp.net[i].weight.detach().numpy()
            out["lin/" + name] = layer_out[name].numpy()
    path = os.path.join(HERE, "reference_ngp_autocast.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")
    print("\n".join(tr.rows))


if __name__ == "__main__":
    main()
