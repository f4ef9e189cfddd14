"""Hash-grid NeRF training (lzzx_nerf_amd/ngp_train.py, csrc/lz_ngp_train.hip) without a device: the module builds with the operator
path's parameters and state-dict keys, refuses what is not built, and the new entry points are declared, exported and bound; argument
errors come back before any launch; no spills, no scratch."""
import ctypes as C
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lz_ngp_head_backward", "lz_ngp_train_workspace")
FAKE = 0x10000   # never dereferenced: every case below is rejected (or a no-op) on the host


def _generic_modules():
    """the modules GenericHashgridNeRF builds (synthetic.py), on the CPU"""
    from lzzx_nerf_amd.encoding import get_encoder
    from lzzx_nerf_amd.linear import MLP
    enc, dim = get_encoder("hashgrid")
    return enc, MLP(dim, 16, 64, 2), MLP(16 + 15, 3, 64, 2)


def test_module_builds_with_the_operator_paths_keys():
    from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF
    enc, sig, col = _generic_modules()
    net = FusedHashgridTrainNeRF()
    want = {"encoder." + k for k in enc.state_dict()} | {"sigma_net." + k for k in sig.state_dict()} | {"color_net." + k for k in col.state_dict()}
    assert set(net.state_dict()) == want
    sd = {"encoder." + k: v for k, v in enc.state_dict().items()}
    sd.update({"sigma_net." + k: v for k, v in sig.state_dict().items()})
    sd.update({"color_net." + k: v for k, v in col.state_dict().items()})
    net.load_state_dict(sd)
    assert torch.equal(net.sigma_net.net[1].weight, sig.net[1].weight) and torch.equal(net.encoder.embeddings, enc.embeddings)
    shared = FusedHashgridTrainNeRF(enc, sig, col)
    assert shared.encoder.embeddings is enc.embeddings and len(list(shared.parameters())) == 5


def test_refusals():
    from lzzx_nerf_amd.encoding import get_encoder
    from lzzx_nerf_amd.linear import MLP
    from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF
    net = FusedHashgridTrainNeRF()
    x, d = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="positions or directions"):
        net(x.clone().requires_grad_(True), d)
    with pytest.raises(RuntimeError, match="positions or directions"):
        net(x, d.clone().requires_grad_(True))
    net.encoder.embeddings.data = net.encoder.embeddings.data.half()
    with pytest.raises(RuntimeError, match="f32 tables"):
        net(x, d)
    with pytest.raises(RuntimeError, match="encoder must be"):
        FusedHashgridTrainNeRF(get_encoder("hashgrid", num_levels=8)[0])
    with pytest.raises(RuntimeError, match="encoder must be"):
        FusedHashgridTrainNeRF(get_encoder("tiledgrid", input_dim=3)[0])
    with pytest.raises(RuntimeError, match="sigma MLP 32-64-16"):
        FusedHashgridTrainNeRF(None, MLP(32, 16, 32, 2))
    torch.set_autocast_enabled("cuda", True)     # what `with torch.autocast("cuda")` switches on (the CPU-only build ignores the context)
    try:
        with pytest.raises(RuntimeError, match="outside torch.autocast"):
            FusedHashgridTrainNeRF()(x, d)
    finally:
        torch.set_autocast_enabled("cuda", False)


def test_new_symbols_declared_exported_bound():
    from test_cabi import _declared
    from lzzx_nerf_amd import _lib
    names = _declared()
    lib = C.CDLL(_lib.SO_PATH)
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _lib.ALL_SYMBOLS, n
    assert _lib.load().lz_ngp_train_workspace() >= 512 * 24 * 256 * 4


def _bwd(null=None, rows=64):
    from lzzx_nerf_amd import _lib
    lib = _lib.load()
    names = ["packed", "ws0", "ws1", "wc0", "wc1", "feats", "dirs", "rows", "count", "g_sigma", "g_rgb", "d_feats", "gs0", "gs1", "gc0", "gc1",
             "workspace", "stream"]
    args = [FAKE] * len(names)
    args[names.index("rows")] = rows
    for n in ("count", "g_sigma", "g_rgb", "stream"):
        args[names.index(n)] = None
    if null:
        args[names.index(null)] = None
    return lib.lz_ngp_head_backward(*args)


@pytest.mark.parametrize("null", ["packed", "ws0", "wc1", "feats", "dirs", "d_feats", "gs0", "gc1", "workspace"])
def test_null_arguments_are_rejected_before_any_launch(null):
    from lzzx_nerf_amd import _lib
    assert _bwd(null) == -2, _lib.load().lz_last_error()


def test_zero_rows_is_a_no_op():
    assert _bwd("packed", rows=0) == 0


def test_kernels_have_no_spills_or_scratch():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))["lz_ngp_train.hip"]
    assert {"_Z22lz_k_ngp_head_backward9LzNgpBwdK", "_Z26lz_k_ngp_head_grad_combinePKfj12LzNgpGradOut"} <= set(res)
    for name, r in res.items():
        assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
    assert res["_Z22lz_k_ngp_head_backward9LzNgpBwdK"]["occupancy"] >= 2
