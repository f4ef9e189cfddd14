"""Wave priorities and single-instruction gaps of the f32 frame kernel lz_k_frame<0, 1, 1>, read from the ISA the build's own flags
produce (tools/isa_census.py), against what the committed switch states imply (lz_head_gather.h: LZF_PRIO_TAIL, LZF_PRIO_YOUNG;
lz_head_slice.h: LZ_SLICE_GAP_FENCE).

A wave's sections run either at its base priority or raised (lz_wave_prio).  Without LZF_PRIO_TAIL one section is raised -- refill, march
and the gather up to its last load: one raise, one drop.  With it three more are: the gather's interpolation behind the loads' wait (a
raise and a drop) and the slice's vector tail with the compositing (a raise behind the last MFMA that holds until the next pass's drop).
LZF_PRIO_YOUNG makes every one of them a choice between two priorities under a scalar branch: twice the instructions.

Figures of the parent, commit 10f1a87 (read there with the same census): 2 s_setprio (2, then 0); 28 intervals between consecutive MFMAs
that hold vector instructions, 17 of them exactly one (5 v_mul_f32 of sigma_net.0's enc_a * att inputs, 12 v_max_i32 of its ReLU); the
folded kernel lz_k_frame<2, 1, 1>: 26 and 15."""
import os
import re
import shutil

import pytest

from tools import isa_census as IC

PARENT_COMMIT = "10f1a87"
PARENT_SETPRIO = [2, 0]
PARENT_SINGLE_GAPS = {"f32": 17, "fold_geo": 15}
PARENT_GAPS = {"f32": 28, "fold_geo": 26}
KERNELS = {"f32": IC.KERNEL_F32, "fold_geo": IC.KERNEL_F32_FOLD}


def _default(header, name):
    """the committed state of a compile-time switch: the value behind its `#ifndef NAME`"""
    from lzzx_nerf_amd import build as B
    src = open(os.path.join(B.CSRC, header)).read()
    m = re.search(r"#ifndef %s\n#define %s (\d+)\n#endif" % (name, name), src)
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    from lzzx_nerf_amd import build as B
    c = B._hipcc()
    if not ((os.path.isabs(c) and os.path.exists(c)) or shutil.which(c)):
        pytest.skip("no hipcc")
    asm = IC.frame_isa(out=str(tmp_path_factory.mktemp("frame_prio") / "lz_frame.s"))
    return {k: IC.kernel_instructions(asm, name) for k, name in KERNELS.items()}


@pytest.fixture(scope="module")
def switches():
    return {"tail": _default("lz_head_gather.h", "LZF_PRIO_TAIL"), "young": _default("lz_head_gather.h", "LZF_PRIO_YOUNG"),
            "gap_fence": _default("lz_head_slice.h", "LZ_SLICE_GAP_FENCE")}


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_setprio_count_is_what_the_switches_imply(isa, switches, kernel):
    prio = IC.setprio(isa[kernel])
    assert len(prio) == (len(PARENT_SETPRIO) + 3 * switches["tail"]) * (1 + switches["young"]), prio
    assert set(prio) == ({0, 1, 2} if switches["young"] else {0, 2}), prio
    if not switches["tail"] and not switches["young"]:
        assert prio == PARENT_SETPRIO


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_raised_sections_are_bracketed(isa, switches, kernel):
    """where the s_setprio stand (with LZF_PRIO_YOUNG the two arms of each choice are laid out apart: only the count above is held)"""
    if switches["young"]:
        return
    ins = isa[kernel]
    at = [i for i, t in enumerate(ins) if t.startswith("s_setprio")]
    prio = IC.setprio(ins)
    mfma = [i for i, t in enumerate(ins) if t.startswith("v_mfma")]
    loads = [i for i, t in enumerate(ins[:mfma[0]]) if t.startswith(("global_load_dword", "buffer_load_dword"))]
    pairs = [i for i in loads if IC.is_table_pair_load(ins[i])][1:]      # (the first 8-byte load is the prologue's)
    assert prio == [2, 0, 2, 0, 2][:len(prio)]                          # raise and drop in turn
    # refill, march, the gather's address work and its loads: raised; dropped behind the last load, ahead of the matrix chain
    assert at[0] < pairs[0] and loads[-1] < at[1] < mfma[0]
    if switches["tail"]:
        # the interpolation: raised behind the wait for the loads, dropped ahead of the first MFMA
        assert at[1] < at[2] < at[3] < mfma[0]
        assert any(t.startswith("s_waitcnt vmcnt(0)") for t in ins[at[1]:at[2]])
        assert sum(t.startswith("v_") for t in ins[at[2]:at[3]]) >= 36          # 36 corner products at the least
        # the slice's vector tail: raised behind the last MFMA, not dropped before the kernel's loop closes
        assert at[4] > mfma[-1] and len(at) == 5
        assert sum(t.startswith("v_fma_f32") for t in ins[at[4]:]) >= 64        # the ind_code k-step stands behind it


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_single_instruction_gaps_do_not_exceed_the_parents(isa, kernel):
    single = IC.single_gaps(isa[kernel])
    assert len(single) <= PARENT_SINGLE_GAPS[kernel], single
    assert len(IC.mfma_gaps(isa[kernel])) <= PARENT_GAPS[kernel]


def test_gap_fence_closes_every_single_gap_of_the_headline_kernel(isa, switches):
    if switches["gap_fence"]:
        assert IC.single_gaps(isa["f32"]) == []
