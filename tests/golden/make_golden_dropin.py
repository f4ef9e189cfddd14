#!/usr/bin/env python3
"""Generate tests/golden/reference_dropin.json: what the REFERENCE's own, unmodified nerf_triplane.network.NeRFNetwork asks of the encoder
factory and what it builds from the answers, with lzzx_nerf_amd/dropin in front of sys.path (build container only; the reference tree is
not part of this repository and nothing at test time imports it).

For opt.torso = False and True the fixture records
  * every `get_encoder(...)` call the constructor makes (network.py:131-166): positional and keyword arguments, the attribute the result
    is stored in, the class and output_dim returned, and the grid type of grid encoders;
  * the constructed network's state_dict contract: key -> [shape, dtype];
  * the input widths the constructor derived from the returned output_dims (in_dim, in_dim_dir, torso_*_in_dim).

tests/test_dropin_reference.py replays the recorded calls on the drop-in modules and holds them to this record.

Run:  python tests/golden/make_golden_dropin.py <reference tree>
"""
import json
import os
import subprocess
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DROPIN = os.path.join(ROOT, "lzzx_nerf_amd", "dropin")
OUT = os.path.join(HERE, "reference_dropin.json")

SCRIPT = textwrap.dedent("""
    import json, sys, types
    sys.path.insert(0, %(dropin)r); sys.path.insert(1, %(root)r); sys.path.insert(2, %(ref)r)
    for name in ("lpips", "trimesh", "mcubes", "cv2", "tensorboardX", "torch_ema", "imageio", "pydub", "numba"):
        try: __import__(name)
        except Exception: sys.modules[name] = types.ModuleType(name)   # absent third-party packages off the hot path
    import encoding
    assert encoding.__file__.startswith(%(dropin)r)
    calls, made = [], []
    factory = encoding.get_encoder
    def recording_get_encoder(*args, **kwargs):
        enc, dim = factory(*args, **kwargs)
        c = dict(args=list(args), kwargs=kwargs, type=type(enc).__module__ + "." + type(enc).__qualname__, output_dim=int(dim))
        if hasattr(enc, "gridtype"):
            c["gridtype"] = enc.gridtype
        calls.append(c)
        made.append(enc)
        return enc, dim
    encoding.get_encoder = recording_get_encoder          # before the reference's `from encoding import get_encoder` binds the name
    from nerf_triplane.network import NeRFNetwork            # reference source, unmodified
    class Opt:
        bound=1; min_near=0.05; density_thresh=10; density_thresh_torso=0.01; exp_eye=True; test_train=False
        smooth_lips=False; torso=%(torso)s; cuda_ray=True; ind_num=10; ind_dim=4; ind_dim_torso=8; train_camera=False
        emb=False; asr_model='deepspeech'; att=2; unc_loss=1; torso_shrink=0.8
    net = NeRFNetwork(Opt())
    children = dict(net.named_children())
    for c, enc in zip(calls, made):
        c["attr"] = next(k for k, m in children.items() if m is enc)
    sd = {k: [list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()}
    dims = {k: int(getattr(net, k)) for k in ("in_dim", "in_dim_dir", "torso_deform_in_dim", "anchor_in_dim", "torso_in_dim") if hasattr(net, k)}
    print("RECORD " + json.dumps(dict(get_encoder_calls=calls, state_dict=sd, dims=dims), sort_keys=True))
""")


def record(ref, torso):
    code = SCRIPT % dict(dropin=DROPIN, root=ROOT, ref=ref, torso=torso)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    line = next(l for l in r.stdout.splitlines() if l.startswith("RECORD "))
    return json.loads(line[len("RECORD "):])


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "nerf_triplane")):
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    fixture = {"torso=%s" % t: record(ref, t) for t in (False, True)}
    with open(OUT, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
