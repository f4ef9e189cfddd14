"""What the f32 frame kernels' source intends, counted in the ISA the build's own flags produce: the MFMAs bit-exactness leaves, the dense
levels' 8-byte paired table loads (lz_head_gather.h: PAIR0), a ReLU of one integer instruction between the MFMAs (lz_head_slice.h:
lz_slice_relu) and 32-bit offsets, not per-lane 64-bit addresses, in the gather.  These are counts, not measurements -- the guard whose
absence let the paired loads drop out of the binary unnoticed (the compiler had split each 8-byte memcpy into two dword loads and sunk them
out of the dense branch).

Figures of this tree (lz_k_frame<0, 1, 1> / lz_k_frame<2, 1, 1>): 337 / 273 MFMAs, 7 / 7 eight-byte loads (6 paired table loads and the
prologue's one), no canonicalising v_max_f32 between the MFMAs, no v_lshl_add_u64 in the gather, no packed f32 operation.  The folded
kernel reaches 273 because the ind_code k-step of colour_net.0 runs on the VALU there too (lz_head_slice.h), which it can without a spill
only in a build without the SLP vectoriser."""
import os
import shutil
import subprocess

import pytest

from tools import isa_census as IC

KERNELS = {"f32": IC.KERNEL_F32, "fold_geo": IC.KERNEL_F32_FOLD}
MFMAS = {"f32": 337, "fold_geo": 273}          # 361 - 24; the folded kernel 64 less
PARENT_8_BYTE_LOADS = 1                         # the prologue's, before the paired table loads existed in the binary


def _hipcc():
    from lzzx_nerf_amd import build as B
    c = B._hipcc()
    return c if (os.path.isabs(c) and os.path.exists(c)) or shutil.which(c) else None


@pytest.fixture(scope="session")
def frame_isa(tmp_path_factory):
    from lzzx_nerf_amd import build as B
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("frame_isa") / "lz_frame.s")
    flags = [f for f in B.FLAGS if not f.startswith("-Rpass")] + B.FILE_FLAGS.get("lz_frame.hip", [])
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "lz_frame.hip"), "-o", out], check=True, capture_output=True)
    asm = open(out).read()
    return {k: IC.kernel_instructions(asm, name) for k, name in KERNELS.items()}


def _mfma_span(ins):
    at = [i for i, t in enumerate(ins) if t.startswith("v_mfma_f32_16x16x4_f32")]
    return at[0], at[-1], len(at)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_mfma_count(frame_isa, kernel):
    assert _mfma_span(frame_isa[kernel])[2] == MFMAS[kernel]


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_dense_pairs_are_8_byte_loads(frame_isa, kernel):
    ins = frame_isa[kernel]
    first_mfma = _mfma_span(ins)[0]
    pairs = [i for i, t in enumerate(ins) if IC.is_table_pair_load(t)]
    assert len(pairs) >= PARENT_8_BYTE_LOADS + 6, len(pairs)
    assert sum(i < first_mfma for i in pairs) >= PARENT_8_BYTE_LOADS + 6     # the gather's: issued ahead of the matrix chain


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_no_canonicalising_max_between_the_mfmas(frame_isa, kernel):
    ins = frame_isa[kernel]
    a, b, _ = _mfma_span(ins)
    assert [t for t in ins[a:b + 1] if IC.is_canonicalising_max(t)] == []


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_no_64_bit_address_arithmetic_in_the_gather(frame_isa, kernel):
    """the gather's table loads: from its first paired load to the last load ahead of the first MFMA (the 6 paired and the 36 per-corner
    loads of the two branches stand together there; the SH partial's loads come after the first MFMA)"""
    ins = frame_isa[kernel]
    first_mfma = _mfma_span(ins)[0]
    pairs = [i for i, t in enumerate(ins[:first_mfma]) if IC.is_table_pair_load(t)][PARENT_8_BYTE_LOADS:]
    loads = [i for i, t in enumerate(ins[:first_mfma]) if t.startswith(("global_load_dword", "buffer_load_dword"))]
    assert pairs, "no paired table load ahead of the matrix chain"
    a, b = pairs[0], loads[-1]
    assert sum(a <= i <= b for i in loads) >= 6 + 36, "the gather's loads do not stand together"
    assert [t for t in ins[a:b + 1] if t.startswith("v_lshl_add_u64")] == []


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_no_packed_f32_when_the_build_turns_the_slp_vectoriser_off(frame_isa, kernel):
    from lzzx_nerf_amd import build as B
    if "-fno-slp-vectorize" not in B.FILE_FLAGS.get("lz_frame.hip", []):
        return                                   # the flag is decided by measurement; without it there is nothing to hold
    assert [t for t in frame_isa[kernel] if t.startswith(("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"))] == []
