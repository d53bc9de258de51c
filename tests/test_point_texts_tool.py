"""CPU suite: the argument handling of tools/vmn_point_texts.py (-decode / -encode, --curve and --params; a modular group, an
unknown curve and every malformed command line are usage errors, status 2; a missing input is status 1), and that
verificatum_vmn_amd.interface has the names of the curve interface beside the modular ones.  No GPU: the tool is driven only as
far as its arguments and its input file."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden


def run_tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vmn_point_texts.py")] + list(args), capture_output=True, text=True,
                          timeout=120)


def test_usage_errors_return_2_and_a_missing_input_1(entry, tmp_path):
    missing, out = str(tmp_path / "missing"), str(tmp_path / "out")
    for mode in ("-decode", "-encode"):
        r = run_tool(mode, "--curve", "P-256", missing, out)
        assert r.returncode == 1 and "no such file" in r.stderr, (mode, r.returncode, r.stderr[-1000:])      # past the arguments
        r = run_tool(mode, "-width", "2", "-keywidth", "2", "--wire", "natural", "--curve", "brainpoolp512r1", missing, out)
        assert r.returncode == 1 and "no such file" in r.stderr, (mode, r.returncode, r.stderr[-1000:])
        r = run_tool(mode, "--curve", "P-257", missing, out)
        assert r.returncode == 2 and "unknown curve" in r.stderr, (mode, r.returncode, r.stderr[-1000:])
        assert run_tool(mode, "--bits", "2048", missing, out).returncode == 2                     # no modular groups here
        assert run_tool(mode, "-width", "0", "--curve", "P-256", missing, out).returncode == 2
        assert run_tool(mode, "-keywidth", "0", "--curve", "P-256", missing, out).returncode == 2
        assert run_tool(mode, missing, out).returncode == 2                                       # no group
        assert run_tool(mode, "--curve", "P-256", missing).returncode == 2                        # no output file
    assert run_tool("--curve", "P-256", missing, out).returncode == 2                             # neither -decode nor -encode
    assert run_tool("-decode", "-encode", "--curve", "P-256", missing, out).returncode == 2
    assert not os.path.exists(out)


def test_the_group_of_a_params_file(entry, tmp_path):
    missing, out, params = str(tmp_path / "missing"), str(tmp_path / "out"), str(tmp_path / "params.json")
    open(params, "w").write(json.dumps({"group": {"kind": "ec", "curve": "secp256k1"}}))
    r = run_tool("-decode", "--params", params, missing, out)
    assert r.returncode == 1 and "no such file" in r.stderr, (r.returncode, r.stderr[-1000:])
    assert run_tool("-decode", "--params", params, "--curve", "P-256", missing, out).returncode == 2
    g, _ = load_golden(512)
    open(params, "w").write(json.dumps({"group": {"kind": "modp", "p": format(g["p"], "x"), "q": format(g["q"], "x"), "g": format(g["g"], "x")}}))
    r = run_tool("-encode", "--params", params, missing, out)
    assert r.returncode == 2 and "curve groups only" in r.stderr, (r.returncode, r.stderr[-1000:])
    for text in ("", "{}", '{"group": 5}', '{"group": {"kind": "ec"}}', '{"group": {"kind": "ec", "curve": 7}}',
                 '{"group": {"kind": "ec", "curve": "P-999"}}'):
        open(params, "w").write(text)
        assert run_tool("-encode", "--params", params, missing, out).returncode == 2, text
    assert run_tool("-encode", "--params", str(tmp_path / "nowhere.json"), missing, out).returncode == 2


def test_the_interface_has_the_names_of_the_curve_interface(vmn):
    from verificatum_vmn_amd import interface
    for name in ("point_encode_length", "encode_point_texts", "decode_point_texts", "read_point_texts", "write_decoded_point_plaintexts",
                 "demo_point_ciphertexts"):
        assert callable(getattr(interface, name)), name
    with pytest.raises(ValueError):
        interface.decode_point_texts([])
    assert vmn.lib().vmn_ec_group_encode_length(None) == 0                  # (no device needed: a null group holds nothing)
