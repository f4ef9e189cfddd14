"""HashgridRenderer(mode="fused", steps_per_pass=S) -- S samples per ray and pass in the cfg2 persistent kernel
(csrc/lz_ngp_frame_spp.hip) -- against the LOOP mode and against fused S = 1 of the same renderer, which the existing cfg2 tests pin bit
for bit to the checker and to the reference's loop.  S is a launch shape only: every comparison is torch.equal on image, image_raw,
weights_sum, depth and ray_counts plus equality of state[5] (the total sample count), for the f32 network, the f16 network and the f32
network on half tables.  The 48 x 48-ray ellipsoid scene and the GenericHashgridNeRF(seed=3) nets are tests/test_gpu_ngp_fused.py's."""
import numpy as np
import pytest
import torch

import ngp_regimes as R
from test_gpu_ngp_fused import KEYS, LZF_CEFF, NETS, _sub, assert_same, nets, scene  # noqa: F401  (nets, scene: module-scoped fixtures)

pytestmark = pytest.mark.gpu
ALL_S = [2, 4, 8, 16]
# test 4: an INPUT, chosen so that many rays of the full ellipsoid end on transmittance partway through a group (the test asserts that on
# the loop's own result before it compares anything); not a tolerance.  The seed-3 network is thin: a ray's transmittance stays above
# 0.3 throughout, at 0.7 about a quarter of the rays end on it with a count that is no multiple of 4 or 8
T_THRESH_CUT = 0.7


def render(net, bits, ro, rd, mode="fused", S=1, ctor=None, **kw):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    ctor = {"bound": 1.0, **(ctor or {})}
    r = HashgridRenderer(net, bits, mode=mode, **({"steps_per_pass": S} if mode == "fused" else {}), **ctor)
    out = {k: v.clone() for k, v in r.render(ro, rd, count_samples=True, **kw).items()}
    torch.cuda.synchronize()
    if mode == "fused" and ro.shape[0]:
        out["S"] = r.last_steps_per_pass
    return out


@pytest.fixture(scope="module")
def refs(nets, scene):
    """(case, precision) -> (loop, fused S = 1): computed once per module, shared by the S of a case, not written into"""
    cache = {}
    cases = dict(A=lambda: dict(bits=scene["holes"], ro=scene["ro"], rd=scene["rd"], kw=dict(max_steps=128)),
                 B=lambda: dict(bits=scene["full"], ro=scene["ro"], rd=scene["rd"], kw=dict(max_steps=16, T_thresh=1e-4)),
                 M13=lambda: dict(bits=scene["full"], ro=scene["ro"], rd=scene["rd"], kw=dict(max_steps=13)),
                 CUT=lambda: dict(bits=scene["full"], ro=scene["ro"], rd=scene["rd"], kw=dict(max_steps=64, T_thresh=T_THRESH_CUT)))

    def get(case, precision):
        if (case, precision) not in cache:
            c = cases[case]()
            cache[(case, precision)] = (c, render(nets[precision], c["bits"], c["ro"], c["rd"], mode="loop", **c["kw"]),
                                        render(nets[precision], c["bits"], c["ro"], c["rd"], S=1, **c["kw"]))
        return cache[(case, precision)]
    return get


def assert_frame(got, loop, one, S=None):
    """a fused frame at S samples per pass == the loop and == fused S = 1: outputs, counts, the total sample count"""
    for want in (loop, one):
        if want is not None:
            assert_same(want, got)
            assert int(got["state"][5]) == int(want["state"][5])
    assert int(got["state"][3]) == 1 and int(got["state"][5]) == int(got["ray_counts"].sum())
    if S is not None:
        assert got["S"] == S


# ---- 1. cap not binding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("S", ALL_S)
def test_spp_cap_not_binding(nets, refs, precision, S):
    """case A: holes bitfield, max_steps 128, the reference's schedule (1, 8)"""
    c, loop, one = refs("A", precision)
    got = render(nets[precision], c["bits"], c["ro"], c["rd"], S=S, **c["kw"])
    assert_frame(got, loop, one, S)
    cnt = loop["ray_counts"]
    assert 8 < int(cnt.max()) < 128 and float(loop["weights_sum"].max()) > 0.5 and int((cnt == 0).sum()) > 0
    assert int((cnt % S != 0).sum()) > 0                        # rays whose last group is short


# ---- 2. cap binding, the reference's cap --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("S", ALL_S)
def test_spp_cap_binding_reference(nets, refs, precision, S):
    """case B: the full ellipsoid, max_steps 16, T_thresh 1e-4: rays stand at the cap, the schedule carries them to C_eff > 16 -- phase 2
    then carries each parked ray fewer than S samples (from cnt_base = max_steps)"""
    c, loop, one = refs("B", precision)
    got = render(nets[precision], c["bits"], c["ro"], c["rd"], S=S, **c["kw"])
    c_eff = int(one["state"][LZF_CEFF])
    assert c_eff > 16 and int(one["state"][9]) > 0 and int(loop["ray_counts"].max()) == c_eff
    assert int(got["state"][LZF_CEFF]) == c_eff and int(got["state"][9]) == int(one["state"][9])
    assert_frame(got, loop, one, S)


# ---- 3. max_steps that is no multiple of S ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("cap", ["reference", "per_ray"])
@pytest.mark.parametrize("S", [4, 8, 16])
def test_spp_max_steps_not_a_multiple(nets, scene, refs, precision, cap, S):
    """max_steps 13 (S = 16: a whole ray is one group that stops at 13).  cap "per_ray": against fused S = 1, and against the loop under
    the schedule (1, 1), whose cap is per ray as well (the class docstring)"""
    c, loop, one = refs("M13", precision)
    if cap == "per_ray":
        one = render(nets[precision], c["bits"], c["ro"], c["rd"], S=1, ctor=dict(cap="per_ray"), **c["kw"])
        loop = render(nets[precision], c["bits"], c["ro"], c["rd"], mode="loop", ctor=dict(n_step_cap=1), **c["kw"])
        assert int(one["ray_counts"].max()) == 13
    got = render(nets[precision], c["bits"], c["ro"], c["rd"], S=S, ctor=dict(cap=cap), **c["kw"])
    assert int((loop["ray_counts"] >= 13).sum()) > 0
    assert_frame(got, loop, one, S)


# ---- 4. termination inside a group --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("S", [4, 8])
def test_spp_termination_inside_a_group(nets, refs, precision, S):
    c, loop, one = refs("CUT", precision)
    cnt, ws = loop["ray_counts"], loop["weights_sum"]
    inside = (cnt % S != 0) & (cnt < 64) & ((1 - ws) < T_THRESH_CUT)
    share = float(inside.float().mean())
    print("rays that end on transmittance inside a group of %d: %.3f of %d" % (S, share, cnt.numel()))
    assert share >= 0.05
    got = render(nets[precision], c["bits"], c["ro"], c["rd"], S=S, **c["kw"])
    assert_frame(got, loop, one, S)


# ---- 5. rays that do not fill the groups --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("n,S", [(1, 2), (1, 16), (5, 16), (37 * 29, 16), ("longest", 2), ("longest", 16)])
def test_spp_ray_counts_that_do_not_fill_the_groups(nets, scene, precision, n, S):
    """a seeded subset (and, next to the seeded single ray, the frame's longest ray alone); the output buffers hold NaN (counts: a
    sentinel) before the frame"""
    from lzzx_nerf_amd.ngp import HashgridRenderer
    if n == "longest":
        best = int(render(nets[precision], scene["holes"], scene["ro"], scene["rd"], mode="loop", max_steps=48)["ray_counts"].argmax())
        ro, rd = scene["ro"][best:best + 1].contiguous(), scene["rd"][best:best + 1].contiguous()
    else:
        ro, rd = _sub(scene, n, n)
    loop = render(nets[precision], scene["holes"], ro, rd, mode="loop", max_steps=48)
    one = render(nets[precision], scene["holes"], ro, rd, S=1, max_steps=48)
    assert n == 1 or float(loop["weights_sum"].max()) > 0.0
    r = HashgridRenderer(nets[precision], scene["holes"], bound=1.0, mode="fused", steps_per_pass=S)
    r.render(ro, rd, max_steps=48, count_samples=True)          # allocates the buffers that are then poisoned
    for k in ("out", "image", "weights_sum", "depth"):
        r._fbuf[k].fill_(float("nan"))
    r._fbuf["ray_counts"].fill_(-12345)
    got = r.render(ro, rd, max_steps=48, count_samples=True)
    torch.cuda.synchronize()
    for k in KEYS:
        assert not bool(torch.isnan(got[k].float()).any()), k
    assert_frame(got, loop, one)
    assert r.last_steps_per_pass == S


# ---- 6. degenerate frames -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 16])
def test_spp_on_no_rays(nets, scene, S):
    e = torch.empty(0, 3, device="cuda")
    for cap in ("reference", "per_ray"):
        o = render(nets["f32"], scene["holes"], e, e, S=S, ctor=dict(cap=cap), max_steps=16)
        assert o["image"].shape == (0, 3) and o["depth"].shape == (0,) and o["ray_counts"].shape == (0,) and int(o["state"][5]) == 0


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("S", [4, 16])
def test_spp_all_rays_miss_the_box(nets, scene, precision, S):
    ro = (scene["ro"][:300] + torch.tensor([0.0, 50.0, 0.0], device="cuda")).contiguous()
    rd = torch.tensor([1.0, 0.0, 0.0], device="cuda").expand(300, 3).contiguous()
    kw = dict(max_steps=32, bg_color=0.25)
    got = render(nets[precision], scene["holes"], ro, rd, S=S, **kw)
    assert_frame(got, render(nets[precision], scene["holes"], ro, rd, mode="loop", **kw), render(nets[precision], scene["holes"], ro, rd, S=1, **kw))
    assert bool((got["image"] == 0.25).all()) and int(got["state"][1]) == 0 and int(got["ray_counts"].sum()) == 0


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("S", [4, 16])
def test_spp_uniform_bitfields(nets, scene, precision, fill, S):
    bits = torch.full_like(scene["full"], fill)
    ro, rd = _sub(scene, 700, 7)
    got = render(nets[precision], bits, ro, rd, S=S, max_steps=24)
    loop = render(nets[precision], bits, ro, rd, mode="loop", max_steps=24)
    assert_frame(got, loop, render(nets[precision], bits, ro, rd, S=1, max_steps=24))
    assert (int(loop["ray_counts"].sum()) == 0) == (fill == 0)


# ---- 7. regimes against the CPU checker ---------------------------------------------------------------------------------------------
SPP_RUNS = [(r, i) for r in ("behind", "cascades", "inside", "odd", "grid512", "axis") for i in range(R.N_RUNS.get(r, 1))]
REG_KEYS = ("image", "image_raw", "depth", "weights_sum", "ray_counts")


def regime_frame(run, net, S):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    from test_gpu_ngp_regimes import nets as regime_nets
    dev = R.GpuOps.to
    r = HashgridRenderer(regime_nets(run.encoder)[net], dev(R.bitfield(run.bits)), bound=run.bound, cascade=run.cascade, grid_size=run.grid_size,
                         aabb=dev(run.aabb), min_near=run.min_near, budget_factor=1, n_step_cap=8, mode="fused", cap="reference", steps_per_pass=S)
    got = r.render(dev(run.ro), dev(run.rd), dt_gamma=run.dt_gamma, max_steps=run.max_steps, T_thresh=run.T_thresh, count_samples=True)
    torch.cuda.synchronize()
    out = {k: got[k].cpu().numpy() for k in REG_KEYS}
    out["ray_counts"] = out["ray_counts"].astype(np.int64)
    out["state"] = got["state"].cpu().numpy()
    assert r.last_steps_per_pass == S
    return out


@pytest.mark.parametrize("S", [4, 16])
@pytest.mark.parametrize("net", ["f32", "half", "f16"])
@pytest.mark.parametrize("regime,index", [pytest.param(r, i, id="%s-%d" % (r, i)) for r, i in SPP_RUNS])
def test_spp_regimes(regime, index, net, S):
    """f32 net and half tables: the CPU checker (np.array_equal); the f16 net: the host loop around its own head, as
    test_gpu_ngp_regimes.py arranges it"""
    from test_gpu_ngp_regimes import assert_equals, host_loop_frame
    run = R.runs(regime)[index]
    want = host_loop_frame(regime, index, "f16") if net == "f16" else R.checker_frame(regime, index, half=net == "half")
    got = regime_frame(run, net, S)
    assert_equals(got, want, REG_KEYS, (run.label, net, S))
    assert int(got["state"][3]) == 1 and int(got["state"][5]) == int(got["ray_counts"].sum()) == int(want["ray_counts"].sum())


# ---- 8. back-to-back frames on one renderer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
def test_spp_changes_between_frames(nets, scene, precision):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    r = HashgridRenderer(nets[precision], scene["holes"], bound=1.0, mode="fused")
    for S, n in ((1, 1000), (8, 700), (0, 1000), (2, 37 * 29), (8, 700)):
        ro, rd = _sub(scene, n, 40 + n)
        r.steps_per_pass = S
        got = {k: v.clone() for k, v in r.render(ro, rd, max_steps=16, count_samples=True).items()}
        torch.cuda.synchronize()
        chosen = r.last_steps_per_pass
        assert chosen == S if S else chosen in (1, 2, 4, 8, 16)
        assert_frame(got, render(nets[precision], scene["holes"], ro, rd, mode="loop", max_steps=16), None)
    r.steps_per_pass = 3
    with pytest.raises(ValueError, match="steps_per_pass"):
        r.render(ro, rd, max_steps=16)


# ---- 9. auto ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("n", [37 * 29, 48 * 48])
def test_spp_auto(nets, scene, precision, n):
    ro, rd = _sub(scene, n, n) if n < 48 * 48 else (scene["ro"], scene["rd"])
    got = render(nets[precision], scene["holes"], ro, rd, S=0, max_steps=48)
    assert got["S"] in (1, 2, 4, 8, 16)
    assert_frame(got, render(nets[precision], scene["holes"], ro, rd, mode="loop", max_steps=48), None)
