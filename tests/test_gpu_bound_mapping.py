"""The box-to-unit mapping `(x + bound) / (2 * bound)` (gridencoder/grid.py:143) at bounds where 2 bound is no power of two: which
arithmetic torch runs it in on the device (the premise), and every path of the package held to that arithmetic through the checker --
operators, the three-plane encoder, the training head's scatter coordinates, the fused heads, the frames and the hash-grid network.
Inputs: tests/bound_cases.py (a fifth of the coordinates differ in the last bit between the candidates, 48 rows flip the cell of some
level; tests/test_bound_mapping_host.py holds the inputs to that on the CPU).  Comparisons are bit for bit unless they say otherwise."""
import functools

import numpy as np
import pytest
import torch

import bound_cases as BC
from conftest import ellipsoid_bitfield, synthetic_camera
from lzzx_nerf_amd._util import call, map01, ptr, stream
from lzzx_nerf_amd.gridencoder import GridEncoder, TriplaneEncoder, grid_encode
from oracle import oracle as O
from oracle.head import TriplaneSpec, encode_x, get_rays, head_forward, head_forward_fp16
from oracle.render import render_inference, render_train_forward

pytestmark = pytest.mark.gpu
F32 = np.float32
B = 1000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------
# a. the premise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_device_division_by_scalar_is_a_reciprocal_multiply(bound):
    """torch on the device, f32 tensor and Python-number bound: the result is one of the two candidates on all 2^22 draws, and it is the
    one the checker (oracle.map01), the Python helper (_util.map01) and the kernels (lz_map01) are written in"""
    draws = BC.draws(bound)
    x = dev(draws)
    got = host((x + bound) / (2 * bound))
    is_div, is_rcp = np.array_equal(got, BC.map01_div(draws, bound)), np.array_equal(got, BC.map01_rcp(draws, bound))
    which = "the true division (map01_div)" if is_div else "the reciprocal multiply (map01_rcp)" if is_rcp else "NEITHER candidate"
    assert is_div != is_rcp, "bound %g: torch on the device computes %s" % (bound, which)
    assert is_rcp, "bound %g: torch on the device computes %s; oracle.map01, _util.map01 and lz_map01 are written as the reciprocal multiply" % (bound, which)
    assert np.array_equal(host(map01(x, bound)), got)
    assert np.array_equal(O.map01(draws, bound), got)
    # a tensor divisor is the other arithmetic: what _util.map01 warns of
    assert np.array_equal(host((x + bound) / torch.full((1,), 2.0 * bound, device="cuda")), BC.map01_div(draws, bound))


@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_grid_encoder_forward_is_grid_encode_of_the_premise(bound):
    """GridEncoder.forward has not moved for its users: its output is grid_encode on the tensor the premise's expression gives"""
    enc = _plane_encoder(bound)
    x = dev(BC.draws(bound)).view(-1, 2)
    unit = (x + bound) / (2 * bound)
    with torch.no_grad():
        want = grid_encode(unit, enc.embeddings, enc.offsets, enc.per_level_scale, enc.base_resolution, False, enc.gridtype_id, enc.align_corners)
        assert torch.equal(enc(x, bound=bound), want)


# ------------------------------------------------------------------------------------------------
# b. operators against the checker
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plane_encoders(bound):
    """three GridEncoders (D 2, C 1: the triplane's planes, desired resolution 512 bound) holding BC.triplane_tables(bound)"""
    P = BC.triplane_tables(bound)
    encs = []
    for n in ("xy", "yz", "xz"):
        e = GridEncoder(input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512 * bound)
        assert np.array_equal(e.offsets.numpy(), P[f"encoder_{n}.offsets"])
        with torch.no_grad():
            e.embeddings.copy_(torch.from_numpy(P[f"encoder_{n}.embeddings"]))
        encs.append(e.cuda())
    return tuple(encs)


def _plane_encoder(bound):
    return _plane_encoders(bound)[0]


def _three(encs, xyz, bound):
    return torch.cat([encs[0](xyz[:, :2], bound=bound), encs[1](xyz[:, 1:], bound=bound), encs[2](xyz[:, [0, 2]], bound=bound)], -1)


@functools.lru_cache(maxsize=None)
def _generic(half=False):
    from test_gpu_ngp import make
    return make(half=half)


@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_plane_encoder_equals_the_checker(bound):
    enc, xyz = _plane_encoder(bound), BC.points(bound, B)
    spec = TriplaneSpec(bound)
    want, _ = O.grid_encode_forward(O.map01(xyz[:, :2], bound), BC.triplane_tables(bound)["encoder_xy.embeddings"], spec.offsets,
                                    spec.per_level_scale, spec.base_resolution)
    with torch.no_grad():
        assert np.array_equal(host(enc(dev(xyz)[:, :2], bound=bound)), want)


@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_hashgrid_encoder_equals_the_checker(bound):
    g, _, _, _ = _generic()
    e, xyz = g.enc, BC.points(bound, B, "cfg2")
    want, _ = O.grid_encode_forward(O.map01(xyz, bound), host(e.embeddings), host(e.offsets), e.per_level_scale, e.base_resolution)
    with torch.no_grad():
        assert np.array_equal(host(e(dev(xyz), bound=bound)), want)


@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
@pytest.mark.parametrize("batch", [65, B])
def test_triplane_encoder_equals_the_three_encoders_and_the_checker(bound, batch):
    encs = _plane_encoders(bound)
    tri = TriplaneEncoder(*encs)
    xyz = BC.points(bound, batch)
    with torch.no_grad():
        got, want = tri(dev(xyz), bound=bound), _three(encs, dev(xyz), bound)
    assert torch.equal(got, want)
    assert np.array_equal(host(got), encode_x(TriplaneSpec(bound), xyz, BC.triplane_tables(bound)))
    if bound == 2.5625:      # the box surface: 1 - 2^-24 is inside the unit interval, the corner rows are not zeroed
        assert bool((got[:3].abs().amax(1) > 0).all())


@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_triplane_jacobian_equals_the_three_encoders(bound):
    """dy_dx of lz_triplane_encode_forward [3, B, L, 2] against lz_grid_encode_forward's [B, L * 2] per plane"""
    encs = _plane_encoders(bound)
    e, L = encs[0], 12
    xyz = dev(BC.points(bound, B))
    S = float(F32(np.log2(e.per_level_scale)))
    out = torch.empty(B, 3 * L, device="cuda")
    jac = torch.zeros(3, B, L, 2, device="cuda")
    call("lz_triplane_encode_forward", ptr(xyz), ptr(encs[0].embeddings), ptr(encs[1].embeddings), ptr(encs[2].embeddings), ptr(e.offsets), ptr(out),
         ptr(jac), B, L, S, int(e.base_resolution), float(bound), stream())
    for plane, cols in enumerate(([0, 1], [1, 2], [0, 2])):
        unit = map01(xyz[:, cols], bound).contiguous()
        o1 = torch.empty(B, L, device="cuda")
        j1 = torch.zeros(B, L * 2, device="cuda")
        call("lz_grid_encode_forward", ptr(unit), ptr(encs[plane].embeddings), ptr(e.offsets), ptr(o1), B, 2, 1, L, S, int(e.base_resolution), ptr(j1),
             0, 0, 0, 1, stream())
        assert bool(j1.any())
        assert torch.equal(out[:, plane * L:(plane + 1) * L], o1), plane
        assert torch.equal(jac[plane].reshape(B, L * 2), j1), plane


# ------------------------------------------------------------------------------------------------
# d. the training head's scatter coordinates
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_plane_coords_are_the_mapping_of_the_column_pairs(bound):
    xyz = BC.points(bound, B)
    out = torch.empty(3, B, 2, device="cuda")
    call("lz_triplane_plane_coords", ptr(dev(xyz)), B, float(bound), ptr(out), stream())
    for plane, cols in enumerate(([0, 1], [1, 2], [0, 2])):
        assert np.array_equal(host(out[plane]), O.map01(xyz[:, cols], bound)), plane


# ------------------------------------------------------------------------------------------------
# e. the fused triplane head
# ------------------------------------------------------------------------------------------------
def _head(p, bound, precision="f32"):
    from lzzx_nerf_amd.head import FusedTriplaneHead
    return FusedTriplaneHead({k: torch.from_numpy(np.asarray(v)) for k, v in p.items()}, bound=bound, precision=precision)


@pytest.mark.parametrize("bound", BC.BOUNDS)
@pytest.mark.parametrize("testing", [True, False])
def test_fused_head_f32_equals_the_checker(params, golden, bound, testing):
    p = BC.triplane_params(params, bound)
    xyz, d = BC.points(bound, B), BC.dirs(B)
    enc_a, eye, ind = golden["net_enc_a"], golden["net_eye"], golden["net_ind"]
    want = head_forward(TriplaneSpec(bound), p, xyz, d, enc_a, ind, eye, testing=testing)
    got = _head(p, bound).forward(dev(xyz), dev(d), dev(enc_a), dev(ind), dev(eye), testing=testing)
    for name, g, w in zip(("sigma", "rgb", "amb_aud", "amb_eye", "unc"), got, want):
        assert np.array_equal(host(g), w), name


@pytest.mark.parametrize("bound", BC.BOUNDS)
def test_fused_head_f16_matches_autocast_checker(params, golden, bound):
    """the comparison and tolerances of test_gpu_parity.test_fused_head_f16_matches_autocast_checker (boost 0, with the eye), unchanged"""
    p = BC.triplane_params(params, bound)
    xyz, d = BC.points(bound, B), BC.dirs(B)
    enc_a, eye, ind = golden["net_enc_a"], golden["net_eye"], golden["net_ind"]
    so, ro, ao, eo, uo = head_forward_fp16(TriplaneSpec(bound), p, xyz, d, enc_a, ind, eye)
    sg, rg, ag, eg, ug = (host(t) for t in _head(p, bound, "f16").forward(dev(xyz), dev(d), dev(enc_a), dev(ind), dev(eye)))
    assert np.array_equal(ug, uo)
    assert np.allclose(rg, ro, atol=4e-3) and np.mean(rg == ro) > 0.85, (np.abs(rg - ro).max(), np.mean(rg == ro))
    assert np.allclose(sg, so, rtol=2e-2) and np.mean(np.abs(sg / so - 1) < 4e-6) > 0.85, (np.abs(sg / so - 1).max(), np.mean(np.abs(sg / so - 1) < 4e-6))
    assert np.allclose(ag, ao, rtol=5e-3, atol=1e-4)
    assert np.allclose(eg, eo, atol=2e-3)


def test_dropin_encoders_equal_the_checker_at_bound_1p5():
    """the drop-in graph of test_gpu_parity.test_dropin_network_path_matches_checker (get_encoder() three times and a cat) at bound 1.5:
    enc_x is the checker's encode_x on the same samples"""
    from lzzx_nerf_amd.encoding import get_encoder
    bound = 1.5
    P = BC.triplane_tables(bound)
    encs = []
    for n in ("xy", "yz", "xz"):
        e, od = get_encoder("hashgrid", input_dim=2, num_levels=12, level_dim=1, base_resolution=64, log2_hashmap_size=14, desired_resolution=512 * bound)
        e = e.cuda()
        e.embeddings.data.copy_(dev(P[f"encoder_{n}.embeddings"]))
        encs.append(e)
    xyz = BC.points(bound, B)
    x = dev(xyz)
    with torch.no_grad():
        enc_x = torch.cat([encs[0](x[:, :2], bound=bound), encs[1](x[:, 1:], bound=bound), encs[2](x[:, [0, 2]], bound=bound)], -1)
    assert np.array_equal(host(enc_x), encode_x(TriplaneSpec(bound), xyz, P))


# ------------------------------------------------------------------------------------------------
# f. triplane frames at bound 1.5: two cascades, 40 x 40 rays, max_steps 48, an ellipsoid per cascade
# ------------------------------------------------------------------------------------------------
FRAME_BOUND, FRAME_HW, FRAME_STEPS = 1.5, 40, 48


@functools.lru_cache(maxsize=None)
def _frame_inputs():
    pose, intr = synthetic_camera(FRAME_HW, FRAME_HW)
    ro, rd = get_rays(pose, intr, FRAME_HW, FRAME_HW)
    bits = np.concatenate([ellipsoid_bitfield()[0], ellipsoid_bitfield(semi=(0.7, 0.4, 0.3))[0]])      # level 0: [-1, 1]^3; level 1: [-1.5, 1.5]^3
    return np.ascontiguousarray(ro), np.ascontiguousarray(rd), bits


def _frame_params(params):
    p = BC.triplane_params(params, FRAME_BOUND)
    w = params["sigma_net.net.2.weight"].copy()
    w[0] *= 40.0                                   # test_gpu_parity._scene: rays terminate, the schedule takes n_step > 1
    p["sigma_net.net.2.weight"] = w
    return p


_CHECKER_FRAMES = {}


def _checker_frame(params, golden, schedule):
    """the checker's frame under (budget_factor, n_step_cap) = schedule, once per process"""
    if schedule not in _CHECKER_FRAMES:
        ro, rd, bits = _frame_inputs()
        st = {}
        ref = render_inference(TriplaneSpec(FRAME_BOUND), _frame_params(params), ro, rd, bits, golden["net_enc_a"], golden["net_ind"], golden["net_eye"],
                               cascade=2, max_steps=FRAME_STEPS, stats=st, budget_factor=schedule[0], n_step_cap=schedule[1])
        cnt = st["samples_per_ray"]
        assert cnt.max() > 8 and (cnt == 0).any() and (ref["weights_sum"] > 0.5).any()       # the frame is a frame
        _CHECKER_FRAMES[schedule] = (ref, st)
    return _CHECKER_FRAMES[schedule]


def _frame_equals(out, ref, st):
    assert np.array_equal(host(out["ray_counts"]).astype(np.int64), st["samples_per_ray"])
    for k in ("image", "depth", "weights_sum", "amb_aud_sum", "amb_eye_sum", "uncertainty_sum"):
        assert np.array_equal(host(out[k]), ref[k]), k


def _frame_args(golden):
    ro, rd, bits = _frame_inputs()
    return dev(bits), (dev(ro), dev(rd), dev(golden["net_enc_a"]), dev(golden["net_ind"]), dev(golden["net_eye"]))


def test_loop_frame_equals_the_checker(params, golden):
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    ref, st = _checker_frame(params, golden, (1, 8))
    bits, args = _frame_args(golden)
    r = TriplaneRenderer(_head(_frame_params(params), FRAME_BOUND), bits, bound=FRAME_BOUND, cascade=2)
    out = r.render(*args, max_steps=FRAME_STEPS, count_samples=True)
    _frame_equals(out, ref, st)
    state = host(out["state"])
    assert state[5] == st["samples_per_ray"].sum() and state[6] == len(st["schedule"]) and state[3] == 1


@pytest.mark.parametrize("cap", ["per_ray", "reference"])
def test_fused_frame_equals_the_checker(params, golden, cap):
    """per_ray with one step per pass is the loop under the schedule (1, 1); reference is the loop under the reference's (1, 8)"""
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    ref, st = _checker_frame(params, golden, (1, 1) if cap == "per_ray" else (1, 8))
    bits, args = _frame_args(golden)
    r = TriplaneRenderer(_head(_frame_params(params), FRAME_BOUND), bits, bound=FRAME_BOUND, cascade=2, mode="fused", cap=cap)
    if cap == "per_ray":
        r.steps_per_pass = 1
    out = r.render(*args, max_steps=FRAME_STEPS, count_samples=True)
    _frame_equals(out, ref, st)


def test_train_forward_equals_the_checker(params, golden):
    """test_gpu_parity.test_train_forward_matches_checker at bound 1.5, two cascades"""
    from lzzx_nerf_amd import raymarching as R
    ro, rd, bits = _frame_inputs()
    p = BC.triplane_params(params, FRAME_BOUND)
    enc_a, eye, ind = golden["net_enc_a"], golden["net_eye"], golden["net_ind"]
    ref = render_train_forward(TriplaneSpec(FRAME_BOUND), p, ro, rd, bits, enc_a, ind, eye, cascade=2, max_steps=FRAME_STEPS, force_all_rays=True)
    b = FRAME_BOUND
    aabb = dev(np.array([-b, -b / 2, -b, b, b / 2, b], F32))
    nears, fars = R.near_far_from_aabb(dev(ro), dev(rd), aabb, 0.05)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, deltas, rays = R.march_rays_train(dev(ro), dev(rd), b, dev(bits), 2, 128, nears, fars, ctr, -1, False, 128, True, 1 / 256, FRAME_STEPS)
    sig, rgb, aa, ae, unc = _head(p, b).forward(xyzs.contiguous(), dirs.contiguous(), dev(enc_a), dev(ind), dev(eye), testing=False)
    ws, a0s, a1s, us, dep, img = R.composite_rays_train_triplane(sig, rgb, aa.abs().sum(-1), ae.abs().sum(-1), unc, deltas, rays)
    c = ref["comp"]
    assert ref["sigmas"].shape[0] > 1000
    assert np.array_equal(host(rays), ref["rays"]) and np.array_equal(host(sig), ref["sigmas"])
    assert np.array_equal(host(ws), c["weights_sum"]) and np.array_equal(host(img), c["image"]) and np.array_equal(host(us), c["unc_sum"])
    assert np.array_equal(host(a0s), c["amb0_sum"]) and np.array_equal(host(a1s), c["amb1_sum"]) and np.array_equal(host(dep), c["depth"])


# ------------------------------------------------------------------------------------------------
# h. the hash-grid network
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", BC.BOUNDS)
@pytest.mark.parametrize("half", [False, True])
def test_fused_hashgrid_net_equals_the_checker(bound, half):
    _, fused, _, cpu_net = _generic(half)
    xyz, d = BC.points(bound, B, "cfg2"), BC.dirs(B)
    sig, rgb = fused.forward(dev(xyz), dev(d), bound)
    sig_c, rgb_c = cpu_net(xyz, d, bound)
    assert np.array_equal(host(sig), sig_c) and np.array_equal(host(rgb), rgb_c)
