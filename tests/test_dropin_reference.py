"""Drop-in check against the reference's own, unmodified caller code, held to a record of it: tests/golden/reference_dropin.json holds
every get_encoder call the reference's nerf_triplane.network.NeRFNetwork constructor makes (with lzzx_nerf_amd/dropin in front of
sys.path), the classes and output_dims it received, and the state_dict contract of the network it built (generated in the build
container by tests/golden/make_golden_dropin.py).  Here, with the drop-in directory in front of sys.path, the reference's import names
must resolve to the drop-in modules, and the recorded calls replayed on them must return the same modules -- class, output_dim, grid type
and state_dict entries -- that the reference's network was built from.  No GPU needed."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_dropin.json")

SCRIPT = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, %(dropin)r); sys.path.insert(1, %(root)r)
    import encoding, raymarching, gridencoder, shencoder, freqencoder
    assert all(m.__file__.startswith(%(dropin)r) for m in (encoding, raymarching, gridencoder, shencoder, freqencoder))
    rec = json.load(open(%(fixture)r))[%(case)r]
    sd = rec["state_dict"]
    for c in rec["get_encoder_calls"]:
        enc, dim = encoding.get_encoder(*c["args"], **c["kwargs"])
        assert type(enc).__module__ + "." + type(enc).__qualname__ == c["type"], (c["attr"], type(enc))
        assert dim == c["output_dim"] == enc.output_dim, (c["attr"], dim)
        assert getattr(enc, "gridtype", None) == c.get("gridtype"), c["attr"]
        mine = {k: [list(v.shape), str(v.dtype)] for k, v in enc.state_dict().items()}
        want = {k[len(c["attr"]) + 1:]: v for k, v in sd.items() if k.startswith(c["attr"] + ".")}
        assert mine == want, (c["attr"], mine, want)
    print('DROPIN_OK', len(sd))
""")


@pytest.fixture(scope="module")
def record():
    return json.load(open(FIXTURE))


@pytest.mark.parametrize("torso", [False, True])
def test_reference_network_constructs_on_dropin(torso, record):
    case = "torso=%s" % torso
    rec = record[case]
    sd, dims = rec["state_dict"], rec["dims"]
    attrs = {c["attr"]: c for c in rec["get_encoder_calls"]}
    # what the reference built on the drop-in modules
    assert attrs["encoder_xy"]["type"].endswith("GridEncoder") and attrs["encoder_dir"]["type"].endswith("SHEncoder")
    assert dims["in_dim"] == 36 and dims["in_dim_dir"] == 16
    assert sd["encoder_xy.embeddings"] == [[163584, 1], "torch.float32"] and sd["encoder_yz.offsets"][1] == "torch.int32"
    assert sd["sigma_net.net.0.weight"][0] == [64, 69] and sd["density_bitfield"][0] == [262144]
    if torso:
        assert attrs["torso_deform_encoder"]["type"].endswith("FreqEncoder") and dims["torso_deform_in_dim"] == 34
        assert attrs["torso_encoder"]["type"].endswith("GridEncoder") and attrs["torso_encoder"]["gridtype"] == "tiled"
        assert dims["torso_in_dim"] == 32
    # the fused head consumes this state_dict as is (construction + packing need a GPU, so only the key contract here)
    from lzzx_nerf_amd import head
    assert all(k in sd for k in head._W_KEYS)
    # ... and the drop-in modules, imported under the reference's names, still answer the recorded calls with the same modules
    code = SCRIPT % dict(dropin=os.path.join(ROOT, "lzzx_nerf_amd", "dropin"), root=ROOT, fixture=FIXTURE, case=case)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DROPIN_OK" in r.stdout, r.stderr[-3000:]
