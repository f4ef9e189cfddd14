"""The order-free table gradient (lz_grid_encode_backward_fixed, gridencoder.set_table_grad("fixed"), csrc/lz_grid_fixed.hip): every term
quantised with one power-of-two scale per level, summed as 64-bit integers, rounded once.  Held to what its definition promises: the same
bits on every call, under a permutation of the rows and in both gradient layouts; the checker's bits on inputs whose sums are exact;
the checker to the quantisation bound otherwise; one f32 add onto the buffer; non-finite gradients where the float scatter puts them; a
workspace that needs no care; and the four followers of the module switch.  Encoders, batches and the checker's results are those of
test_gpu_grid_ordered.py and test_gpu_exact_grid_scatter.py (computed once, shared, read-only)."""
import copy
import functools

import numpy as np
import pytest
import torch

import exact_inputs as E
from lzzx_nerf_amd import _lib, gridencoder
from lzzx_nerf_amd._util import call, ptr, stream
from test_gpu_grid_ordered import SIZES, _bits, _d_feats, _data, _encoder, _fused, _hyper, _oracle, _points, _reference, _table_grad_of

pytestmark = pytest.mark.gpu

NAMES = ["d3_t17", "d3_t8", "plane", "tiled_ac"]          # the encoders of test_gpu_grid_ordered.py with C <= 2


def _entry(h, x, g, layout=1, out=None, ws=None, dy_dx=None, stride=0, check=True):
    """lz_grid_encode_backward_fixed straight from the C ABI on cuda tensors; h: dict(D, C, L, S, H, gridtype, ac, offsets (cuda), shape).
    g: [B, L*C] (turned into [L, B, C] for layout 0).  A fresh workspace is filled with a byte pattern: the call has to clear it."""
    B = x.shape[0]
    if layout == 0:
        g = g.view(B, h["L"], h["C"]).permute(1, 0, 2).contiguous()
    ge = torch.zeros(h["shape"], device="cuda") if out is None else out
    need = int(_lib.load().lz_grid_fixed_workspace(h["shape"][0], h["C"]))
    if ws is None:
        ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    jac = gi = None
    if dy_dx is not None:
        jac, gi = torch.from_numpy(np.array(dy_dx, dtype=np.float32)).cuda().contiguous(), torch.zeros(B, h["D"], device="cuda")
    rc = _lib.load().lz_grid_encode_backward_fixed(ptr(g), ptr(x), None, ptr(h["offsets"]), ptr(ge), B, h["D"], h["C"], h["L"], h["S"], h["H"],
                                                   ptr(jac), ptr(gi), h["gridtype"], int(h["ac"]), 0, layout, ptr(ws), need & 0xFFFFFFFF, need >> 32,
                                                   stride, stream())
    if check:
        _lib.check(rc, "lz_grid_encode_backward_fixed")
    torch.cuda.synchronize()
    return ge, gi


@functools.lru_cache(maxsize=None)
def _h(name):
    h = _hyper(_encoder(name))
    h["offsets"] = torch.from_numpy(h["offsets"]).cuda()
    return h


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda().contiguous()          # a copy: the shared inputs are read-only


def _run(name, x, g, **kw):
    return _entry(_h(name), _cuda(x), _cuda(g), **kw)[0]


def _level_scales(g, B, D, L, C):
    """e per level from the definition (None: nothing to add or the float path); g [B, L*C]"""
    hb = max(2, int(np.ceil(np.log2(B * 2 ** D))))
    out = []
    for lvl in range(L):
        a = np.abs(g[:, lvl * C:(lvl + 1) * C])
        m = np.float32(np.inf) if np.isnan(a).any() else np.float32(a.max(initial=0.0))
        if m == 0 or not np.isfinite(m):
            out.append(None)
            continue
        ex = int(np.frexp(m)[1])                                     # m < 2^ex
        out.append(int(np.clip(51 - hb - ex, -100, 100)))
    return out


# ---- 1. a function of the SET of samples ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_same_bits_for_any_order_layout_and_call(name, B):
    x, g = _data(name, B)
    perm = np.random.default_rng(7 + B).permutation(B)
    first = None
    for label, (xx, gg) in (("as given", (x, g)), ("permuted", (x[perm], g[perm]))):
        for layout in (0, 1):
            for call_no in (1, 2):
                got = _bits(_run(name, xx, gg, layout=layout))
                if first is None:
                    first = got
                    assert first.any()
                n = int((got != first).sum())
                print(name, B, label, "layout", layout, "call", call_no, "entries that differ:", n, "of", first.size)
                assert n == 0, (name, B, label, layout, call_no)


def test_the_checker_itself_depends_on_the_permutation():
    """the guard on the inputs (CPU only): on d3_t8 at B = 4099 the checker gives other bits for the permuted batch, so the property above
    is one that an order-following sum does not have"""
    name, B = "d3_t8", 4099
    x, g = _data(name, B)
    perm = np.random.default_rng(7 + B).permutation(B)
    a, b = _bits(_reference(name, B)), _bits(_oracle(name, x[perm].copy(), g[perm].copy())[0])
    print("entries whose bits differ under the permutation:", int((a != b).sum()), "of", a.size)
    assert (a != b).sum() > 0.25 * a.size


# ---- 2. exact inputs: the checker's bits ------------------------------------------------------------------------------------------
EXACT = [(n, B) for n in E.GRID_CASES if E.GRID_CASES[n][2] <= 2 for B in E.GRID_BATCHES[n]]


@pytest.mark.parametrize("name,B", EXACT)
def test_exact_inputs_equal_the_checker_bit_for_bit(name, B):
    from test_gpu_exact_grid_scatter import bits, dev, encoder, reference, where_off
    D, L, C, H, T, gt, _ = E.GRID_CASES[name]
    enc = encoder(name)
    ge, touched = reference(name, B)
    assert touched.any() and (~touched).any()
    x, g = E.grid_inputs(name, B)
    h = dict(D=D, C=C, L=L, S=1.0, H=H, gridtype=0 if gt == "hash" else 1, ac=False, offsets=enc.offsets, shape=tuple(enc.embeddings.shape))
    for layout in (0, 1):
        gemb = torch.zeros_like(enc.embeddings.data)
        for launch in (1, 2):
            _entry(h, dev(x), dev(g), layout=layout, out=gemb)
            got = gemb.cpu().numpy()
            want = ge * np.float32(launch)
            assert np.array_equal(bits(got), bits(want)), "layout %d launch %d: " % (layout, launch) + where_off(got, want)
        assert not bits(got)[~touched].any()          # entries no sample touches: +0, not even -0


# ---- 3. random inputs: the checker to the bound of the definition ------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_close_to_the_checker(name, B):
    """|fixed - checker| <= 2^-23 2^D B max|g| (any f32 order of the terms, the atomic test's bound) + 2^D B 2^-(e+1) (the quantisation:
    half a unit of 2^-e per term, at most 2^D B terms), e from the definition per level"""
    h = _h(name)
    D, L, C = h["D"], h["L"], h["C"]
    x, g = _data(name, B)
    ref = _reference(name, B).astype(np.float64)
    got = _run(name, x, g).cpu().numpy().astype(np.float64)
    off = h["offsets"].cpu().numpy()
    es = _level_scales(g, B, D, L, C)
    for lvl, e in enumerate(es):
        assert e is not None
        bound = 2.0 ** -23 * 2 ** D * B * float(np.abs(g).max()) + 2 ** D * B * 2.0 ** -(e + 1)
        err = float(np.abs(got[off[lvl]:off[lvl + 1]] - ref[off[lvl]:off[lvl + 1]]).max())
        print(name, B, "level", lvl, "e", e, "error", err, "bound", bound)
        assert err <= bound, (name, B, lvl, err, bound)


@pytest.mark.parametrize("name", ["d3_t8", "tiled_ac"])
def test_grad_inputs_are_the_checkers(name):
    from oracle import oracle as O
    enc = _encoder(name)
    x, g = _data(name, 4099)
    _, jac = O.grid_encode_forward(x, enc.embeddings.detach().numpy(), enc.offsets.numpy(), enc.per_level_scale, enc.base_resolution, True,
                                   enc.gridtype_id, enc.align_corners)
    _, gi_ref = _oracle(name, x, g, jac)
    plain = _bits(_run(name, x, g))
    for layout in (0, 1):
        ge, gi = _entry(_h(name), _cuda(x), _cuda(g), layout=layout, dy_dx=jac)
        assert np.array_equal(_bits(ge), plain) and np.array_equal(_bits(gi), _bits(gi_ref)), (name, layout)


# ---- 4. one f32 add onto what the buffer holds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("d3_t17", 257), ("d3_t8", 4099), ("plane", 4099), ("tiled_ac", 63)])
def test_adds_onto_the_buffer_and_leaves_the_rest(name, B):
    x, g = _data(name, B)
    zeros = _run(name, x, g).cpu().numpy()
    pattern = np.random.default_rng(5).standard_normal(zeros.shape).astype(np.float32)
    pattern.reshape(-1)[::7] = -0.0
    got = _run(name, x, g, out=_cuda(pattern)).cpu().numpy()
    written = _bits(zeros) != 0
    want = np.where(written, pattern + zeros, pattern)
    assert written.any()
    if name == "d3_t17":
        assert (~written & (_bits(pattern) == 0x80000000)).any()          # a -0.0 that no term reaches
    assert np.array_equal(_bits(got), _bits(want))


# ---- 5. non-finite gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("name,level", [("d3_t17", 0), ("d3_t17", 9), ("plane", 3)])
def test_a_non_finite_gradient_poisons_its_entries_and_no_other_level(name, level, bad):
    from oracle import oracle as O
    enc = _encoder(name)
    h = _h(name)
    C, B, row = h["C"], 4099, 1234
    x, g = _data(name, B)
    assert (x[row] >= 0).all() and (x[row] <= 1).all()
    g = g.copy()
    ch = C - 1
    g[row, level * C + ch] = bad
    clean = _run(name, *_data(name, B)).cpu().numpy()
    got = _run(name, x, g).cpu().numpy()
    idx = O.grid_corner_indices(x, enc.offsets.numpy(), C, enc.per_level_scale, enc.base_resolution, enc.gridtype_id, enc.align_corners)
    hit = idx[level, row].astype(np.int64) + ch                        # element offsets of the entries the sample touches at that level
    assert (hit >= 0).all()
    assert not np.isfinite(got.reshape(-1)[hit]).any()
    off = h["offsets"].cpu().numpy()
    other = np.ones(got.shape[0], dtype=bool)
    other[off[level]:off[level + 1]] = False
    assert np.array_equal(_bits(got)[other], _bits(clean)[other])
    inside = got[off[level]:off[level + 1]]
    assert np.isfinite(inside).sum() > 0                                # the float path reached the level's other entries too
    ref = _reference(name, B)[off[level]:off[level + 1]]
    ok = np.isfinite(inside)
    assert np.abs(inside[ok] - ref[ok]).max() <= 2.0 ** -23 * 8 * B * float(np.abs(_data(name, B)[1]).max())


# ---- 6. the workspace needs no care -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d3_t17", "plane"])
def test_two_batches_on_one_workspace(name):
    h = _h(name)
    ws = torch.empty(int(_lib.load().lz_grid_fixed_workspace(h["shape"][0], h["C"])), dtype=torch.uint8, device="cuda")
    for B in (4099, 257, 70001, 4099):
        x, g = _data(name, B)
        fresh = _bits(_run(name, x, g))
        shared = _bits(_run(name, x, g, ws=ws))
        assert np.array_equal(fresh, shared), (name, B)


def test_a_workspace_sized_for_fewer_entries_is_not_a_gradient():
    """offsets live on the device, so a workspace that holds the first levels only is found there: those levels are summed, the others add
    nothing and carry a NaN in their first element"""
    name, B = "d3_t8", 257
    h = _h(name)
    off = h["offsets"].cpu().numpy()
    x, g = _data(name, B)
    full = _run(name, x, g).cpu().numpy()
    short = int(_lib.load().lz_grid_fixed_workspace(int(off[5]), h["C"]))
    ws = torch.empty(short, dtype=torch.uint8, device="cuda")
    ge = torch.zeros(h["shape"], device="cuda")
    gd = _cuda(g)
    rc = _lib.load().lz_grid_encode_backward_fixed(ptr(gd), ptr(_cuda(x)), None, ptr(h["offsets"]), ptr(ge), B, h["D"], h["C"], h["L"], h["S"], h["H"], None,
                                                   None, h["gridtype"], 0, 0, 1, ptr(ws), short, 0, 0, stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = ge.cpu().numpy()
    assert np.array_equal(_bits(got[:off[5]]), _bits(full[:off[5]]))
    for lvl in range(5, h["L"]):
        assert np.isnan(got[off[lvl], 0]) and not got[off[lvl]:off[lvl + 1]].reshape(-1)[1:].any()


# ---- 7. the followers of the switch -----------------------------------------------------------------------------------------------
@pytest.fixture
def fixed():
    prev = gridencoder.set_table_grad("fixed")
    yield
    gridencoder.set_table_grad(prev)


def test_grid_encoder_follows_the_switch(fixed, monkeypatch):
    name, B = "d3_t17", 4099
    enc = copy.deepcopy(_encoder(name)).cuda()
    x01, g = _data(name, B)
    pts = (torch.from_numpy(x01.copy()) * 2 - 1).cuda()
    gd = _cuda(g)
    calls = []
    real = gridencoder.grid_backward_fixed
    monkeypatch.setattr(gridencoder, "grid_backward_fixed", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    enc(pts).backward(gd)
    assert len(calls) == 1
    want, _ = _entry(_h(name), ((pts + 1) / 2).contiguous(), gd)
    assert np.array_equal(_bits(enc.embeddings.grad), _bits(want)) and _bits(want).any()
    # with grad_inputs: the same table gradient, positions' gradient as under "atomic"
    enc.embeddings.grad = None
    p2 = pts.clone().requires_grad_(True)
    enc(p2).backward(gd)
    assert np.array_equal(_bits(enc.embeddings.grad), _bits(want))
    gridencoder.set_table_grad("atomic")
    p3 = pts.clone().requires_grad_(True)
    enc(p3).backward(gd)
    gridencoder.set_table_grad("fixed")
    assert torch.equal(p2.grad, p3.grad)
    # half tables (autocast, even level_dim) are refused with the mode that serves them
    enc.embeddings.grad = None
    with torch.autocast("cuda", dtype=torch.float16):
        out = enc(pts)
    assert out.dtype == torch.float16
    with pytest.raises(RuntimeError, match="f32 tables only.*atomic"):
        out.backward(gd.half())


def test_unsupported_encoders_are_refused_with_the_modes_that_serve(fixed):
    for name, word in (("c4", "ordered"), ("c8", "ordered")):
        enc = copy.deepcopy(_encoder(name)).cuda()
        x01, g = _data(name, 257)
        out = enc((torch.from_numpy(x01.copy()) * 2 - 1).cuda())
        with pytest.raises(RuntimeError, match=word):
            out.backward(_cuda(g))


@pytest.mark.parametrize("M", [1, 257, 4099])
def test_triplane_encoder_follows_the_switch(fixed, M):
    from lzzx_nerf_amd.gridencoder import TriplaneEncoder
    encs = tuple(copy.deepcopy(_encoder("plane")).cuda() for _ in range(3))
    tri = TriplaneEncoder(*encs)
    gen = torch.Generator().manual_seed(60 + M)
    xyz = torch.rand(M, 3, generator=gen) * 2 - 1
    if M >= 8:
        xyz[3, 0], xyz[4, 1], xyz[5, 2], xyz[M - 1] = 1.25, -1.5, 1 + 2.0 ** -20, torch.tensor([-1.0, 0.5, 1.0])     # outside, and on the surface
    xyz = xyz.cuda()
    g = torch.randn(M, 36, generator=gen).cuda()
    tri(xyz, bound=1).backward(g)
    unit = ((xyz + 1) / 2)
    h = _h("plane")
    for p, cols in enumerate(((0, 1), (1, 2), (0, 2))):
        want, _ = _entry(h, unit[:, list(cols)].contiguous(), g[:, 12 * p:12 * p + 12].contiguous())
        assert np.array_equal(_bits(encs[p].embeddings.grad), _bits(want)), (M, p)
        assert _bits(want).any()


@pytest.mark.parametrize("M", [1, 257, 4099])
def test_training_head_follows_the_switch(fixed, params, golden, M):
    from lzzx_nerf_amd.head_train import FusedTriplaneTrainHead
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(11 + M)
    xyz = ((torch.rand(M, 3, device="cuda", generator=gen) * 2 - 1) * torch.tensor([1.0, 0.5, 1.0], device="cuda")).contiguous()
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda", generator=gen), dim=-1)
    up = [torch.randn(M, device="cuda", generator=gen), torch.randn(M, 3, device="cuda", generator=gen)] + \
         [torch.randn(M, 1, device="cuda", generator=gen) for _ in range(3)]
    net = FusedTriplaneTrainHead({k: v for k, v in params.items()}, bound=1.0).cuda()          # f32, recorded
    net.keep_denc = True
    outs = net(xyz, dirs, dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))
    sum((o * u).sum() for o, u in zip(outs, up)).backward()
    x01 = torch.empty(3, M, 2, device="cuda")
    call("lz_triplane_plane_coords", ptr(xyz), M, 1.0, ptr(x01), stream())
    for p, enc in enumerate((net.encoder_xy, net.encoder_yz, net.encoder_xz)):
        h = dict(D=2, C=1, L=12, S=net.S, H=net.H, gridtype=0, ac=False, offsets=net.offsets, shape=tuple(enc.embeddings.shape))
        d = net.last_denc[p].contiguous()                                  # [12, M]: what the scatter was fed, level-major
        want, _ = _entry(h, x01[p].contiguous(), d.t().contiguous(), layout=0)
        assert np.array_equal(_bits(enc.embeddings.grad), _bits(want)), (M, p)
        assert _bits(want).any()


@pytest.fixture(scope="module")
def generic():
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    return GenericHashgridNeRF("cuda", seed=3)


@pytest.mark.parametrize("M", [1, 257, 4099])
def test_fused_hashgrid_net_follows_the_argument_and_the_switch(generic, M):
    net = _fused(generic, "fixed")
    xyzs, dirs, gs, gr = _points(M, 40 + M)
    a = _table_grad_of(net, xyzs, dirs, gs, gr)
    b = _table_grad_of(net, xyzs, dirs, gs, gr)
    assert np.array_equal(_bits(a), _bits(b))
    d = _d_feats(net, xyzs, dirs, gs, gr).permute(1, 0, 2).reshape(M, 32).contiguous()
    e = net.encoder
    h = dict(D=3, C=2, L=16, S=net._S, H=net._H, gridtype=0, ac=False, offsets=e.offsets, shape=tuple(e.embeddings.shape))
    want, _ = _entry(h, ((xyzs + 1.0) / 2.0).contiguous(), d, layout=0)
    assert np.array_equal(_bits(a), _bits(want)) and _bits(want).any()
    follow = _fused(generic, None)
    prev = gridencoder.set_table_grad("fixed")
    try:
        c = _table_grad_of(follow, xyzs, dirs, gs, gr)
    finally:
        gridencoder.set_table_grad(prev)
    assert np.array_equal(_bits(c), _bits(a))
