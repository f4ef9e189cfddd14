"""The hash-grid NeRF in the reference's autocast arithmetic, pinned on the CPU: tests/ngp_fp16_checker.py against the reference's own
GridEncoder / SHEncoder / MLP run under torch autocast (tests/golden/reference_ngp_autocast.npz, make_golden_ngp_autocast.py), and the
f16 head's weight image (lzzx_nerf_amd/ngp.py: pack_weights_f16) and register budget.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import ngp_fp16_checker as K
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
F16, F32 = np.float16, np.float32

# the aten ops under the autocast layer of make_golden_ngp_autocast.py's run, with their dtypes: the policy the fixture documents.
# Where CUDA autocast differs (exp: fp32 list there) the checker follows CUDA; a torch whose CPU autocast changes any line fails here.
OP_TRACE = [
    "add.Tensor(float32)->float32", "div.Tensor(float32)->float32",           # GridEncoder.forward: (x + bound) / (2 bound)
    "_to_copy.default(float32)->float16",                                      # grid.py:38-39: half table (is_autocast_enabled patched)
    "copy_.default(float16,float16)->float16", "permute.default(float16)->float16", "_unsafe_view.default(float16)->float16",
    "_to_copy.default(float32)->float16", "mm.default(float16,float16)->float16", "relu_.default(float16)->float16",   # sigma_net
    "_to_copy.default(float32)->float16", "mm.default(float16,float16)->float16",
    "select.int(float16)->float16", "exp.default(float16)->float16",           # CPU: half -> half; CUDA: fp32 list
    "div.Tensor(float32)->float32", "copy_.default(float32,float32)->float32",  # SHEncoder in f32
    "slice.Tensor(float16)->float16", "_to_copy.default(float16)->float32", "cat.default(float32,float32)->float32",   # cat promotes
    "_to_copy.default(float32)->float16", "_to_copy.default(float32)->float16", "mm.default(float16,float16)->float16",   # colour_net
    "relu_.default(float16)->float16", "_to_copy.default(float32)->float16", "mm.default(float16,float16)->float16",
    "sigmoid.default(float16)->float16",
]


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "reference_ngp_autocast.npz"))


def _weights(G):
    return {n: G["w/" + n] for n in K.LAYERS}


def test_table_recipe_reproduces_the_checksum(G):
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    g = GenericHashgridNeRF(torch.device("cpu"), seed=int(G["table_seed"]))
    emb = g.enc.embeddings.detach().numpy()
    assert tuple(emb.shape) == tuple(G["table_shape"])
    assert emb.astype(np.float64).sum() == float(G["table_sum_f64"]) and np.abs(emb.astype(np.float64)).sum() == float(G["table_abssum_f64"])
    assert np.array_equal(emb[G["table_idx"]], G["table_rows"])
    assert np.array_equal(g.enc.offsets.cpu().numpy(), G["offsets"])
    for n, lin in (("sigma_net.net.0", g.sigma_net.net[0]), ("sigma_net.net.1", g.sigma_net.net[1]), ("color_net.net.0", g.color_net.net[0]),
                   ("color_net.net.1", g.color_net.net[1])):
        assert np.array_equal(lin.weight.detach().numpy(), G["w/" + n]), n
    # and the checker's half gather of that table is the reference encoder's output under autocast
    f = K.features(emb, G["offsets"], float(G["per_level_scale"]), G["xyz"], float(G["bound"]))
    assert f.dtype == F16 and np.array_equal(f.view(np.int16), G["feats"].view(np.int16))
    assert 0 < int((f == 0).all(1).sum()) < f.shape[0] // 2       # some positions outside the bound: zero features


def test_checker_linear_layers_bit_for_bit(G):
    tr = {}
    K.head(_weights(G), G["feats"], G["dirs"], tr)
    for n in K.LAYERS:
        want = G["lin/" + n]
        assert want.dtype == F16 and tr[n].dtype == F16 and tr[n].shape == want.shape, n
        assert np.array_equal(tr[n].view(np.int16), want.view(np.int16)), (n, int((tr[n] != want).sum()))


def test_checker_sigma_is_f32_exp_of_the_half_preactivation(G):
    sigma, _ = K.head(_weights(G), G["feats"], G["dirs"])
    pre = G["lin/sigma_net.net.1"][:, 0]
    assert sigma.dtype == F32 and np.array_equal(sigma, O.unary("exp", pre.astype(F32)))
    # the CPU run's own exp is half -> half (not CUDA's policy): the same value rounded to half
    assert G["sigma"].dtype == F16 and int(K.half_ulps(sigma.astype(F16), G["sigma"]).max()) <= 1


def test_checker_rgb_bit_for_bit(G):
    _, rgb = K.head(_weights(G), G["feats"], G["dirs"])
    assert rgb.dtype == F16 and np.array_equal(rgb.view(np.int16), G["rgb"].view(np.int16))
    assert len(np.unique(rgb)) > 50                   # not a constant output


class _Trace(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.rows = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.__name__
        if name.split(".")[0] in ("mm", "exp", "cat", "sigmoid", "relu_"):
            dt = lambda x: [str(y.dtype).replace("torch.", "") for y in (x if isinstance(x, (list, tuple)) else [x]) if isinstance(y, torch.Tensor)]
            self.rows.append("%s(%s)->%s" % (name, ",".join(d for a in args for d in dt(a)), ",".join(dt(out))))
        return out


def test_recorded_op_policy_is_the_documented_one(G):
    assert list(G["op_trace"]) == OP_TRACE
    assert bool(G["autocast_query_patched"])
    # and this torch's CPU autocast still applies that policy to the head's ops (nn.Linear, relu, exp, cat, sigmoid)
    W = _weights(G)
    lin = {n: torch.nn.Linear(W[n].shape[1], W[n].shape[0], bias=False) for n in K.LAYERS}
    with torch.no_grad():
        for n in K.LAYERS:
            lin[n].weight.copy_(torch.from_numpy(W[n]))
    sh, _ = O.sh_encode_forward(G["dirs"], 4)
    tr = _Trace()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16), tr:
        h = lin["sigma_net.net.1"](torch.relu_(lin["sigma_net.net.0"](torch.from_numpy(G["feats"]))))
        torch.exp(h[:, 0])
        c = lin["color_net.net.1"](torch.relu_(lin["color_net.net.0"](torch.cat([torch.from_numpy(sh), h[:, 1:]], -1))))
        torch.sigmoid(c)
    keep = [r for r in OP_TRACE if r.split(".")[0] in ("mm", "exp", "cat", "sigmoid", "relu_")]
    assert tr.rows == keep


# ---- the f16 head's weight image and register budget ----

def test_pack_weights_f16_places_every_half_weight_once():
    """every half weight exactly once where lz_k_ngp_head16's lane map reads it, everything else zero: the image is decoded with the
    kernel's own operand map (fragment (ks, ft), lane (r, h), element j = W[tile row 32 ft + r][k slot 16 ks + 8 h + j], w_chain for
    chained operands, sigma at tile row 4, colour channels at rows 0 / 4 / 1)"""
    from lzzx_nerf_amd.ngp import COLOUR_ROWS, NGP_FRAGS_F16, SIGMA_ROW, pack_weights_f16
    shapes = [(64, 32), (16, 64), (64, 31), (3, 64)]
    sig_out = {SIGMA_ROW: 0, 0: SIGMA_ROW}

    def chain(ks, h, j):
        return 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3)
    bases, nts, kss = (0, 4, 8, 12), (2, 1, 2, 1), (2, 4, 2, 4)
    for L in range(4):
        # one layer at a time, its weights numbered 1, 2, ... (<= 2048: exact in half), the others zero
        ws = [torch.zeros(sh) for sh in shapes]
        ws[L] = torch.arange(1, shapes[L][0] * shapes[L][1] + 1, dtype=torch.float32).reshape(shapes[L])
        img = pack_weights_f16(*ws).cpu().numpy()
        assert img.dtype == F16 and img.size * 2 == 16384 == NGP_FRAGS_F16 * 64 * 16
        img = img.reshape(NGP_FRAGS_F16, 64, 8)
        seen = np.zeros(ws[L].numel(), np.int64)
        mine = np.zeros(img.shape, bool)
        for ks in range(kss[L]):
            for ft in range(nts[L]):
                f = bases[L] + ks * nts[L] + ft
                for lane in range(64):
                    r, h = lane & 31, lane >> 5
                    trow = 32 * ft + r
                    for j in range(8):
                        if L == 0:
                            want = (trow, 16 * ks + 8 * h + j)
                        elif L == 1:
                            want = (sig_out.get(trow, trow), chain(ks, h, j)) if trow < 16 else None
                        elif L == 2:
                            o = sig_out.get(chain(0, h, j), chain(0, h, j))
                            want = (trow, 8 * h + j) if ks == 0 else ((trow, 16 + o - 1) if o >= 1 else None)
                        else:
                            want = (COLOUR_ROWS.index(trow), chain(ks, h, j)) if trow in COLOUR_ROWS else None
                        mine[f, lane, j] = True
                        v = float(img[f, lane, j])
                        if want is None:
                            assert v == 0, (L, ks, ft, lane, j)
                            continue
                        assert v == ws[L][want].item(), (L, ks, ft, lane, j, v)
                        seen[int(v) - 1] += 1
        assert (seen == 1).all(), L                     # every weight exactly once
        assert not img[~mine].any(), L                  # nothing in the other layers' fragments
    # the rounding is autocast's cast of an f32 weight: nearest even, once
    g = torch.Generator().manual_seed(0)
    w = [torch.rand(sh, generator=g) - 0.5 for sh in shapes]
    img = pack_weights_f16(*w).cpu().numpy()
    want = np.concatenate([x.half().numpy().ravel() for x in w])
    assert sorted(img[img != 0].tolist()) == sorted(want[want != 0].tolist())


def test_f16_head_precision_arguments():
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    g = GenericHashgridNeRF(torch.device("cpu"))
    with pytest.raises(ValueError):
        FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, half_tables=False, precision="f16")
    with pytest.raises(ValueError):
        FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, precision="bf16")
    for kw, half, packed16 in ((dict(), False, False), (dict(half_tables=True), True, False), (dict(precision="f16"), True, True),
                               (dict(precision="f16", half_tables=True), True, True)):
        f = FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, **kw)
        assert f.half_tables == half and (f.packed16 is not None) == packed16 and f.table.dtype == (torch.float16 if half else torch.float32)


def test_f16_head_kernel_resources():
    """lz_k_ngp_head16 (build.py's kernel_resources.json): no spill, no scratch, the 16 KB half image in LDS, five waves per SIMD"""
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))["lz_ngp.hip"]
    names = [k for k in res if k.startswith("_Z15lz_k_ngp_head16")]
    assert len(names) == 1, names
    r = res[names[0]]
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, r
    assert r["vgprs"] <= 82 and r["occupancy"] >= 5 and r["lds"] == 16384, r
