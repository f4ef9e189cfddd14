#!/usr/bin/env python3
"""Instruction census of one kernel by source section: copies csrc/ to a scratch directory, plants `; LZMARK name` comments at the given
source anchors, compiles to ISA and counts instructions between the markers (the slices are straight-line code, so static = dynamic).
Markers move a little with instruction scheduling: read neighbouring sections together.

    python tools/isa_census.py            # the f16 fused frame kernel lz_k_frame<1, 1, 2>
    python tools/isa_census.py --f32      # the f32 one, lz_k_frame<0, 1, 1> (the headline launch), by the sections of lz_head_slice.h
    python tools/isa_census.py --gaps [-DLZF_PRIO_TAIL=1 ...]   # both f32 frame kernels: vector instructions between MFMAs, s_setprio

The summary line counts, over the whole kernel, four things the source intends and a compiler can quietly undo: 8-byte table loads (the
dense levels' paired corners), packed f32 vector ops (the SLP vectoriser's), canonicalising v_max_f32 (both sources the same register:
what a float ReLU on an MFMA result costs extra) and v_lshl_add_u64 (a per-lane 64-bit address where a 32-bit offset was meant).
"""
import collections
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lzzx_nerf_amd", "csrc")
TMP = "/tmp/lz_census"
KERNEL_F16 = "_Z10lz_k_frameILi1ELi1ELi2EEvN7LzfHeadIXT_EE4ArgsE8LzFrameK"
KERNEL_F32 = "_Z10lz_k_frameILi0ELi1ELi1EEvN7LzfHeadIXT_EE4ArgsE8LzFrameK"
KERNEL_F32_FOLD = "_Z10lz_k_frameILi2ELi1ELi1EEvN7LzfHeadIXT_EE4ArgsE8LzFrameK"

_GATHER = [("    bool oobc[3];", "g_pos"), ("    uint32_t rowH[2][3][2]", "g_rows"), ("    float gv[9][4];", "g_loads"),
           ('    asm volatile("" ::"v"(gv[0][0])', "g_pin"), ("    if constexpr (PACK) {", "g_interp")]
_FRAME = [("            int ray = slot_lane ? sloti[SF_RAY * NS + sl] : -1;\n            bool have = false;", "F_refill_march"),
          ("            typename HD::Out o;\n            if constexpr (PREC == 1) {", "F_head"),
          ("            __builtin_amdgcn_wave_barrier();     // the parked outputs", "F_composite")]
# the f32 slice (lz_head_slice.h): gather positions / loads / interpolation (lz_head_gather.h), audio, eye, sigma, colour, tail; the
# march and the compositing are the frame's own sections
MARKS_F32 = {
    "lz_head_slice.h": [("    float att[LZ_T][8];", "audio"), ("    float eyeatt[LZ_T];", "eye"), ("    float geo[LZ_T][16];", "sigma"),
                        ("    float rgb[LZ_T][3];", "colour"), ("    out.sigma = sig_pre[0];", "tail")],
    "lz_head_gather.h": _GATHER,
    "lz_frame.hip": _FRAME,
}
MARKS = {
    "lz_head_f16w_slice.h": [("    lz_h8 bx[3];\n", "gather"), ("    lz_h8 att16[2];   // [u][j]", "aud"), ("    {   // ambient_aud = || att ||_2", "norm"),
                             ("    float eyeatt = 0.0f;", "eye"), ("    lz_h8 geo16[4];", "sigma"), ("        lz_h8 b1[6];\n", "colour"),
                             ("    out.eyeatt = eyeatt;", "end")],
    "lz_head_gather.h": _GATHER,
    "lz_frame.hip": _FRAME,
}


def kernel_instructions(asm, kernel):
    """the instructions of one kernel's body in program order, labels, directives and comments dropped"""
    i = asm.index(kernel + ":")
    out = []
    for line in asm[i:asm.index(".Lfunc_end", i)].split("\n"):
        t = line.split(";")[0].strip()
        if t and t[0] != "." and not t.endswith(":"):
            out.append(t)
    return out


def is_table_pair_load(t):
    return re.match(r"(global|buffer)_load_dwordx2\b", t) is not None


def is_canonicalising_max(t):
    m = re.match(r"v_max_f32(?:_e32|_e64)?\s+\S+,\s*(\S+),\s*(\S+)$", t)
    return m is not None and m.group(1) == m.group(2)


def is_packed_f32(t):
    return re.match(r"v_pk_\w+_f32\b", t) is not None


def summary_counts(ins):
    return {"loads_8_byte": sum(map(is_table_pair_load, ins)), "v_pk_f32": sum(map(is_packed_f32, ins)),
            "canonicalising_v_max_f32": sum(map(is_canonicalising_max, ins)), "v_lshl_add_u64": sum(t.startswith("v_lshl_add_u64") for t in ins)}


def mfma_gaps(ins):
    """[(number of the MFMA in front, [vector instructions that are no MFMA])] for every interval between two consecutive MFMAs of the kernel
    that holds any.  Beside f32 MFMAs, opening such a gap costs more than each further instruction in it (tools/probes): the intervals
    with exactly one instruction are the ones worth closing."""
    at = [i for i, t in enumerate(ins) if t.startswith("v_mfma")]
    out = []
    for n, (a, b) in enumerate(zip(at, at[1:])):
        v = [t for t in ins[a + 1:b] if t.startswith("v_")]
        if v:
            out.append((n, v))
    return out


def single_gaps(ins):
    return [(n, v[0]) for n, v in mfma_gaps(ins) if len(v) == 1]


def setprio(ins):
    """the kernel's s_setprio instructions in program order, as their priorities"""
    return [int(t.split()[1]) for t in ins if t.startswith("s_setprio")]


def frame_isa(extra_flags=(), out=None):
    """lz_frame.hip compiled to ISA with the library's own flags (the f32 compilation) and `extra_flags` (-D switches)"""
    sys.path.insert(0, ROOT)
    from lzzx_nerf_amd import build as B
    out = out or os.path.join(TMP + "_isa", "lz_frame.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    flags = [f for f in B.FLAGS if not f.startswith("-Rpass")] + B.FILE_FLAGS.get("lz_frame.hip", []) + list(extra_flags)
    subprocess.run([B._hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "lz_frame.hip"), "-o", out], check=True, capture_output=True)
    return open(out).read()


def gaps_report(extra_flags):
    """--gaps [-DSWITCH=V ...]: per f32 frame kernel the intervals between MFMAs that hold vector instructions, the single ones by name"""
    asm = frame_isa(extra_flags)
    for kernel in (KERNEL_F32, KERNEL_F32_FOLD):
        ins = kernel_instructions(asm, kernel)
        gaps = mfma_gaps(ins)
        one = single_gaps(ins)
        print("%s: %d MFMAs, %d intervals with vector instructions, %d with exactly one, s_setprio %s" % (
            kernel, sum(t.startswith("v_mfma") for t in ins), len(gaps), len(one), setprio(ins)))
        for n, t in one:
            print("    behind MFMA %3d: %s" % (n, t))


def main():
    if "--gaps" in sys.argv:
        return gaps_report([a for a in sys.argv[1:] if a.startswith("-D")])
    pos = [a for a in sys.argv[1:] if not a.startswith("-")]
    f32 = "--f32" in sys.argv
    KERNEL = pos[0] if pos else (KERNEL_F32 if f32 else KERNEL_F16)
    marks_by_file = MARKS_F32 if f32 else MARKS
    shutil.rmtree(TMP, ignore_errors=True)
    shutil.copytree(SRC, TMP)
    for f, marks in marks_by_file.items():
        p = os.path.join(TMP, f)
        s = open(p).read()
        for anchor, name in marks:
            if anchor not in s:
                print("anchor not found:", f, name, file=sys.stderr)
                continue
            i = s.index(anchor)
            ls = s.rfind("\n", 0, i) + 1
            s = s[:ls] + '    asm volatile("; LZMARK %s");\n' % name + s[ls:]
        open(p, "w").write(s)
    out = os.path.join(TMP, "k.s")
    sys.path.insert(0, ROOT)
    from lzzx_nerf_amd import build as B          # the library's own flags, the per-file ones included
    flags = [f for f in B.FLAGS if not f.startswith("-Rpass")] + B.FILE_FLAGS.get("lz_frame.hip", [])
    if KERNEL.startswith("_Z10lz_k_frameILi1E"):      # the f16 frame kernels are the source's second compilation
        flags += B.FILE_PARTS["lz_frame.hip"]["f16"]
    subprocess.run([B._hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(TMP, "lz_frame.hip"), "-o", out], check=True, capture_output=True)
    s = open(out).read()
    i = s.index(KERNEL + ":")
    body = s[i:s.index(".Lfunc_end", i)].split("\n")
    sec, cnt, ops = "prologue", collections.OrderedDict(), collections.OrderedDict()
    for line in body:
        t = line.strip()
        m = re.match(r"; LZMARK (\w+)", t)
        if m:
            sec = m.group(1)
            continue
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        kind = ("mfma" if "mfma" in op else "valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "lds" if op.startswith("ds_")
                else "vmem" if op.startswith(("global_", "buffer_", "flat_")) else "other")
        cnt.setdefault(sec, collections.Counter())[kind] += 1
        if kind == "valu":
            ops.setdefault(sec, collections.Counter())[op] += 1
    tot = collections.Counter()
    for k, v in cnt.items():
        print("%-16s %s" % (k, dict(v)))
        if k not in ("prologue", "F_refill_march", "F_composite"):
            tot.update(v)
    print("slice total (F_head .. end):", dict(tot))
    print("kernel summary:", summary_counts(kernel_instructions(s, KERNEL)))
    if "-v" in sys.argv:
        for k, v in ops.items():
            print(k, dict(v.most_common()))


if __name__ == "__main__":
    main()
