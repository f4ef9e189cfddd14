"""tests/bound_cases.py on the CPU checker alone: the batches the GPU tests of the box-to-unit mapping run on do tell the two candidate
arithmetics apart -- last bits on a fifth of the coordinates and, on dedicated rows, the cell of some level -- and at power-of-two
bounds nothing distinguishes them.  Prints its shares and counts (run with -s)."""
import numpy as np
import pytest

import bound_cases as BC
from oracle import oracle as O
from oracle.head import TriplaneSpec, encode_x

F32 = np.float32
B = 1000


@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_triplane_batch_tells_the_candidates_apart(bound):
    xyz = BC.points(bound, B)
    div, rcp = BC.map01_div(xyz, bound), BC.map01_rcp(xyz, bound)
    share = float((div != rcp).mean())
    found = len(BC.flips("triplane", bound))
    rows, cols = BC.flip_rows("triplane", bound, B)
    spec, P = TriplaneSpec(bound), BC.triplane_tables(bound)
    fd, fr = BC.encode_x_with(BC.map01_div, spec, xyz, P), BC.encode_x_with(BC.map01_rcp, spec, xyz, P)
    print("bound %g: candidates differ on %.3f of the coordinates; %d cell-flipping draws of 2^22, %d placed; %.3f of the feature values differ"
          % (bound, share, found, len(rows), float((fd != fr).mean())))
    assert share >= 0.2
    assert found >= 16 and len(rows) >= 16
    scales = BC.level_scales("triplane", bound)
    placed = xyz[rows, cols]
    flipped = np.zeros(len(rows), bool)
    for s in scales:
        flipped |= BC.cells(BC.map01_div(placed, bound), s) != BC.cells(BC.map01_rcp(placed, bound), s)
    assert flipped.all()
    assert (np.abs(placed) < F32(bound)).all()                      # inside the box: no feature is zeroed
    assert (fd[rows] != fr[rows]).any(1).all()                      # the checker's features differ on every cell-flipping row
    # the rows test_gpu_triplane_encoder.points places
    b = F32(bound)
    assert (xyz[0] == b).all() and (xyz[1] == -b).all() and xyz[3, 0] > b and xyz[4, 1] < -b and xyz[5, 2] > b and xyz[5, 2] - b <= b * F32(2.0 ** -19)
    # the checker's own mapping is one of the two, and its encode_x is that candidate's
    own = O.map01(xyz, bound)
    assert np.array_equal(own, div) != np.array_equal(own, rcp)
    assert np.array_equal(encode_x(spec, xyz, P), fd if np.array_equal(own, div) else fr)


@pytest.mark.parametrize("bound", BC.ENCODER_BOUNDS)
def test_cfg2_batch_tells_the_candidates_apart(bound):
    xyz = BC.points(bound, B, "cfg2")
    share = float((BC.map01_div(xyz, bound) != BC.map01_rcp(xyz, bound)).mean())
    found = len(BC.flips("cfg2", bound))
    rows, cols = BC.flip_rows("cfg2", bound, B)
    pls = np.exp2(np.log2(BC.CFG2["desired_resolution"] / BC.CFG2["base_resolution"]) / (BC.CFG2["num_levels"] - 1))
    offsets = O.grid_offsets(3, 16, pls, 16, 12)                    # a 2^12 table keeps the host test small: the cells are the same
    emb = np.random.default_rng(3).uniform(-1, 1, (int(offsets[-1]), 2)).astype(F32)
    fd, _ = O.grid_encode_forward(BC.map01_div(xyz, bound), emb, offsets, pls, 16)
    fr, _ = O.grid_encode_forward(BC.map01_rcp(xyz, bound), emb, offsets, pls, 16)
    print("cfg2, bound %g: candidates differ on %.3f of the coordinates; %d cell-flipping draws of 2^22, %d placed; %.3f of the feature values differ"
          % (bound, share, found, len(rows), float((fd != fr).mean())))
    assert share >= 0.2
    assert found >= 16 and len(rows) >= 16
    assert (fd[rows] != fr[rows]).any(1).all()


def test_surface_of_the_box_at_2_5625():
    """x = +bound maps to exactly 1 by division and to 1 - 2^-24 by the reciprocal multiply; neither leaves [0, 1]"""
    b = F32(2.5625)
    assert BC.map01_div(b, 2.5625) == F32(1) and BC.map01_rcp(b, 2.5625) == F32(1) - F32(2.0 ** -24)
    for bound in BC.ENCODER_BOUNDS:
        for m in (BC.map01_div, BC.map01_rcp):
            assert m(F32(bound), bound) <= 1 and m(-F32(bound), bound) == 0


@pytest.mark.parametrize("bound", [0.5, 1, 2, 4])
def test_power_of_two_bounds_keep_the_bits_of_the_old_expression(bound):
    x = BC.draws(1.5)[: 1 << 20] * F32(bound / 1.5 * 1.25)          # a quarter of them outside the box
    old = (np.asarray(x, F32) + F32(bound)) / F32(2 * bound)        # what oracle/head.py and oracle/ngp.py spelled out before
    assert np.array_equal(BC.map01_div(x, bound), old) and np.array_equal(BC.map01_rcp(x, bound), old)
    assert np.array_equal(O.map01(x, bound), old)
