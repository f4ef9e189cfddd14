"""HashgridRenderer(mode="fused")'s options / lz_ngp_frame_render_opts and lz_ngp_frame_finish (csrc/lz_ngp_frame.hip): what can be
checked without a GPU -- the declared / exported / bound symbols, the argument rules that return before any launch, the Python-side
checks, and the register, LDS and wave report of the fifteen ngp frame kernels, which now read a ray's march end from t_end under
occupancy clipping."""
import ctypes as C
import json
import os

import pytest
import torch

SYMBOLS = ("lz_ngp_frame_render_opts", "lz_ngp_frame_finish")
BAD_ARGUMENT, UNSUPPORTED = -2, -1


def _renderer(**kw):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    return HashgridRenderer(None, torch.zeros(128 ** 3 // 8, dtype=torch.uint8), **kw)


def _lib():
    from lzzx_nerf_amd import _lib
    return _lib, _lib.load()


def test_symbols_declared_exported_bound():
    from test_cabi import _declared
    L, lib = _lib()
    for s in SYMBOLS:
        assert s in _declared() and s in L.ALL_SYMBOLS and hasattr(C.CDLL(L.SO_PATH), s)
    assert lib.lz_abi_version() == 11
    assert list(lib.lz_ngp_frame_render_opts.argtypes) == [C.POINTER(L.FrameNgpFused), C.POINTER(L.FrameNgpFusedOpts), C.c_uint32, C.c_void_p, C.c_void_p]
    assert list(lib.lz_ngp_frame_finish.argtypes) == [C.POINTER(L.FrameNgpFused), C.POINTER(L.FrameNgpFusedOpts), C.c_uint32, C.c_void_p]
    # the mirror of lz_frame_ngp_fused_opts: four pointers and a word, padded to the pointers' alignment
    assert [n for n, _ in L.FrameNgpFusedOpts._fields_] == ["noises", "occupied_aabb", "t_end", "out_rgb24", "defer_finish"]
    assert C.sizeof(L.FrameNgpFusedOpts) == 40 and L.FrameNgpFusedOpts.defer_finish.offset == 32
    assert C.sizeof(L.FrameNgpFused) == 248                     # lz_frame_ngp_fused keeps its layout


@pytest.mark.parametrize("S", [0, 1, 4, 16])
def test_null_or_zero_options_are_the_plain_entry(S):
    """o == NULL and an all-zero o come back exactly as lz_ngp_frame_render_spp does, refusals included"""
    L, lib = _lib()
    for o in (None, C.byref(L.FrameNgpFusedOpts())):
        f = L.FrameNgpFused()
        assert lib.lz_ngp_frame_render_opts(C.byref(f), o, S, None, None) == 0           # N == 0: nothing to do
        assert lib.lz_ngp_frame_render_opts(None, o, S, None, None) == BAD_ARGUMENT
        f.N = 16
        assert lib.lz_ngp_frame_render_opts(C.byref(f), o, S, None, None) == BAD_ARGUMENT  # null buffers
        want = lib.lz_last_error()
        assert lib.lz_ngp_frame_render_spp(C.byref(f), S, None, None) == BAD_ARGUMENT and lib.lz_last_error() == want
        f.N, f.cap_mode, f.max_steps = 0, 1, 4097
        assert lib.lz_ngp_frame_render_opts(C.byref(f), o, S, None, None) == UNSUPPORTED
        f.max_steps, f.precision = 16, 2
        assert lib.lz_ngp_frame_render_opts(C.byref(f), o, S, None, None) == BAD_ARGUMENT


@pytest.mark.parametrize("bad", [3, 32, 17])
def test_bad_steps_per_pass_is_refused_before_any_launch(bad):
    L, lib = _lib()
    f, o = L.FrameNgpFused(), L.FrameNgpFusedOpts()
    f.N, f.cap_mode = 16, 1
    for call in (lambda: lib.lz_ngp_frame_render_opts(C.byref(f), C.byref(o), bad, None, None), lambda: lib.lz_ngp_frame_finish(C.byref(f), C.byref(o), bad, None),
                 lambda: lib.lz_ngp_frame_render_opts(None, None, bad, None, None), lambda: lib.lz_ngp_frame_finish(None, None, bad, None)):
        assert call() == BAD_ARGUMENT
        assert "steps_per_pass" in lib.lz_last_error().decode()


@pytest.mark.parametrize("N", [0, 16])
def test_argument_rules_name_the_field(N):
    """occupied_aabb without t_end; defer_finish under cap_mode 0; lz_ngp_frame_finish under cap_mode 0 -- each before any launch (no
    device here: a launch would come back as a HIP error), whatever N is"""
    L, lib = _lib()
    box = (C.c_float * 6)()
    f, o = L.FrameNgpFused(), L.FrameNgpFusedOpts()
    f.N = N
    o.occupied_aabb = C.addressof(box)
    for cap_mode in (0, 1):
        f.cap_mode = cap_mode
        assert lib.lz_ngp_frame_render_opts(C.byref(f), C.byref(o), 1, None, None) == BAD_ARGUMENT
        msg = lib.lz_last_error().decode()
        assert "occupied_aabb" in msg and "t_end" in msg
    assert lib.lz_ngp_frame_finish(C.byref(f), C.byref(o), 1, None) == BAD_ARGUMENT and "t_end" in lib.lz_last_error().decode()
    f, o = L.FrameNgpFused(), L.FrameNgpFusedOpts()
    f.N, f.cap_mode, o.defer_finish = N, 0, 1
    assert lib.lz_ngp_frame_render_opts(C.byref(f), C.byref(o), 1, None, None) == BAD_ARGUMENT
    msg = lib.lz_last_error().decode()
    assert "defer_finish" in msg and "cap_mode" in msg
    o.defer_finish = 0
    for opts in (C.byref(o), None):
        assert lib.lz_ngp_frame_finish(C.byref(f), opts, 1, None) == BAD_ARGUMENT
        msg = lib.lz_last_error().decode()
        assert "ngp_frame_finish" in msg and "cap_mode" in msg


def test_empty_and_incomplete_descriptors():
    L, lib = _lib()
    f, o = L.FrameNgpFused(), L.FrameNgpFusedOpts()
    f.cap_mode, o.defer_finish = 1, 1
    assert lib.lz_ngp_frame_render_opts(C.byref(f), C.byref(o), 0, None, None) == 0      # an empty tile without buffers: nothing to do
    assert lib.lz_ngp_frame_finish(C.byref(f), C.byref(o), 0, None) == 0
    assert lib.lz_ngp_frame_finish(C.byref(f), None, 0, None) == 0
    assert lib.lz_ngp_frame_finish(None, None, 0, None) == BAD_ARGUMENT
    f.N = 16
    assert lib.lz_ngp_frame_render_opts(C.byref(f), C.byref(o), 0, None, None) == BAD_ARGUMENT   # null buffers
    assert lib.lz_ngp_frame_finish(C.byref(f), C.byref(o), 0, None) == BAD_ARGUMENT
    f.max_steps = 4097
    assert lib.lz_ngp_frame_finish(C.byref(f), C.byref(o), 0, None) == UNSUPPORTED


def test_renderer_attributes_and_construction():
    from lzzx_nerf_amd.renderer import TriplaneRenderer
    r = _renderer(mode="fused")
    assert (r.clip_to_occupancy, r.occupancy_margin, r.frame_rays_total, r.cap_exchange) == (False, 8, None, None)
    assert _renderer(mode="fused", clip_to_occupancy=True).clip_to_occupancy is True
    with pytest.raises(ValueError, match="clip_to_occupancy"):
        _renderer(mode="loop", clip_to_occupancy=True)
    with pytest.raises(ValueError, match="clip_to_occupancy"):
        _renderer(clip_to_occupancy=True)
    assert _renderer().clip_to_occupancy is False                   # mode "loop" carries the attribute, switched off
    for name in ("occupied_bounds", "invalidate_occupancy", "fused_begin", "fused_finish"):
        assert callable(getattr(r, name))
    assert type(r).occupied_bounds is TriplaneRenderer.occupied_bounds      # one caching rule: tensor identity plus version
    r._occ = object()
    r.invalidate_occupancy()
    assert r._occ is None


def test_python_side_refusals():
    """raised before anything reaches the library (CPU tensors: nothing here could run)"""
    rays = torch.zeros(8, 3)
    for mode in ("loop", "fused"):
        r = _renderer(mode=mode)
        for bad in (torch.zeros(7), torch.zeros(9), torch.zeros(8, 2)):
            with pytest.raises(RuntimeError, match="noises must hold one value per ray"):
                r.render(rays, rays, noises=bad)
    r = _renderer(mode="fused")
    with pytest.raises(RuntimeError, match="noises must hold one value per ray"):
        r.fused_begin(rays, rays, noises=torch.zeros(3))
    with pytest.raises(RuntimeError, match="fused"):
        _renderer(mode="loop").fused_begin(rays, rays)
    r.steps_per_pass = 3
    with pytest.raises(ValueError, match="steps_per_pass"):
        r.fused_begin(rays, rays)


def test_sharded_frame_configure_sets_the_attributes():
    """dist.ShardedFrame.configure drives a HashgridRenderer by the attributes it drives a TriplaneRenderer by"""
    from lzzx_nerf_amd.dist import ShardedFrame
    r = _renderer(mode="fused", cap="per_ray")
    sf = ShardedFrame(48, 48, 0, 1, device="cpu", steps_per_pass=8, cap="reference")
    assert sf.configure(r) is r and (r.cap, r.steps_per_pass, r.frame_rays_total, r.cap_exchange) == ("reference", 8, None, None)
    sf.world = 4                                                    # what a rank of a four-rank frame is handed
    sf.configure(r)
    assert r.frame_rays_total == 48 * 48 and r.cap_exchange == sf.sum_over_ranks
    sf.cap = "per_ray"
    sf.configure(r)
    assert (r.cap, r.frame_rays_total, r.cap_exchange) == ("per_ray", None, None)


def test_to_inference_passes_clip_to_occupancy_through():
    from lzzx_nerf_amd.ngp_train import FusedHashgridTrainNeRF
    net = FusedHashgridTrainNeRF()
    bits = torch.zeros(128 ** 3 // 8, dtype=torch.uint8)
    assert net.to_inference(mode="fused", density_bitfield=bits, clip_to_occupancy=True).clip_to_occupancy is True
    assert net.to_inference(precision="f16", mode="fused", density_bitfield=bits).clip_to_occupancy is False
    with pytest.raises(ValueError, match="clip_to_occupancy"):
        net.to_inference(density_bitfield=bits, clip_to_occupancy=True)     # mode "loop"


# registers, LDS and waves per SIMD of the fifteen kernels: DESIGN 4.5's table.  The kernels read the march end of a ray through a new
# branch on two more kernel arguments (occ, t_end); that may cost neither a vector spill, nor scratch, nor a wave
TABLE = {("frame", 0, "f"): (138, 34896, 3), ("frame", 0, "6__half"): (115, 34896, 3), ("frame", 1, "6__half"): (127, 33616, 2),
         ("spp", 0, "f"): (143, 37456, 3), ("spp", 0, "6__half"): (119, 37456, 3), ("spp", 1, "6__half"): (131, 36688, 2)}


def test_kernel_resources_hold_the_table():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    rows = {}
    for (kind, prec, tt), want in TABLE.items():
        if kind == "frame":
            rows["_Z14lz_k_ngp_frameILi%dE%sEv14LzNgpFrameArgs8LzFrameK" % (prec, tt)] = (res["lz_ngp_frame.hip"], want)
        else:
            for S in (2, 4, 8, 16):
                rows["_Z18lz_k_ngp_frame_sppILi%dE%sLi%dEEv14LzNgpFrameArgs8LzFrameK" % (prec, tt, S)] = (res["lz_ngp_frame_spp.hip"], want)
    assert len(rows) == 15
    for name, (table, (vgprs, lds, waves)) in rows.items():
        r = table[name]
        assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
        assert r["occupancy"] >= waves and r["lds"] <= lds and r["vgprs"] <= vgprs, (name, r, (vgprs, lds, waves))
