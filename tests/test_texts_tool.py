"""CPU suite: the argument handling of tools/vmn_texts.py (-decode / -encode, the group arguments of tools/vmnc_convert.py and
--params; a curve group, a group of another cofactor and every malformed command line are usage errors, status 2), and that
verificatum_vmn_amd.interface keeps refusing `native` as a plaintext format beside the new names.  No GPU: the tool is driven
only as far as its arguments and its input file."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden

import encode_cases as ec


def run_tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vmn_texts.py")] + list(args), capture_output=True, text=True,
                          timeout=120)


def test_usage_errors_return_2_and_a_missing_input_1(entry, tmp_path):
    missing, out = str(tmp_path / "missing"), str(tmp_path / "out")
    for mode in ("-decode", "-encode"):
        r = run_tool(mode, "--bits", "2048", missing, out)
        assert r.returncode == 1 and "no such file" in r.stderr, (mode, r.returncode, r.stderr[-1000:])      # past the arguments
        r = run_tool(mode, "-width", "2", "-keywidth", "2", "--wire", "natural", "--bits", "3072", missing, out)
        assert r.returncode == 1 and "no such file" in r.stderr, (mode, r.returncode, r.stderr[-1000:])
        r = run_tool(mode, "--curve", "P-256", missing, out)
        assert r.returncode == 2 and "modular groups only" in r.stderr, (mode, r.returncode, r.stderr[-1000:])
        assert run_tool(mode, "--bits", "1000", missing, out).returncode == 2                     # no such standard group
        assert run_tool(mode, "-width", "0", "--bits", "2048", missing, out).returncode == 2
        assert run_tool(mode, "-keywidth", "0", "--bits", "2048", missing, out).returncode == 2
        assert run_tool(mode, missing, out).returncode == 2                                       # no group
        assert run_tool(mode, "--bits", "2048", "--curve", "P-256", missing, out).returncode == 2
        assert run_tool(mode, "--bits", "2048", missing).returncode == 2                          # no output file
    assert run_tool("--bits", "2048", missing, out).returncode == 2                               # neither -decode nor -encode
    assert run_tool("-decode", "-encode", "--bits", "2048", missing, out).returncode == 2
    assert not os.path.exists(out)


def test_the_group_of_a_params_file(entry, tmp_path):
    missing, out, params = str(tmp_path / "missing"), str(tmp_path / "out"), str(tmp_path / "params.json")
    g, _ = load_golden(512)
    record = lambda p, q, gen: {"group": {"kind": "modp", "p": format(p, "x"), "q": format(q, "x"), "g": format(gen, "x")}}
    open(params, "w").write(json.dumps(record(g["p"], g["q"], g["g"])))
    r = run_tool("-decode", "--params", params, missing, out)
    assert r.returncode == 1 and "no such file" in r.stderr, (r.returncode, r.stderr[-1000:])
    open(params, "w").write(json.dumps(record(ec.COFACTOR_P, ec.COFACTOR_Q, ec.COFACTOR_G)))
    r = run_tool("-decode", "--params", params, missing, out)
    assert r.returncode == 2 and "p = 2q + 1" in r.stderr, (r.returncode, r.stderr[-1000:])
    open(params, "w").write(json.dumps({"group": {"kind": "ec", "curve": "P-256"}}))
    r = run_tool("-encode", "--params", params, missing, out)
    assert r.returncode == 2 and "modular groups only" in r.stderr, (r.returncode, r.stderr[-1000:])
    for text in ("", "{}", '{"group": 5}', '{"group": {"kind": "modp", "p": "zz"}}'):
        open(params, "w").write(text)
        assert run_tool("-encode", "--params", params, missing, out).returncode == 2, text
    assert run_tool("-encode", "--params", str(tmp_path / "nowhere.json"), missing, out).returncode == 2


def test_the_interface_has_the_new_names_and_keeps_refusing_native(vmn, tmp_path):
    from verificatum_vmn_amd import interface
    assert interface.PLAINTEXT_FORMATS == ("json", "raw")
    with pytest.raises(ValueError):
        interface.write_plaintexts(str(tmp_path / "x"), [object()], "native")
    for name in ("encode_length", "encode_texts", "decode_texts", "write_decoded_plaintexts", "read_texts", "demo_texts", "demo_ciphertexts"):
        assert callable(getattr(interface, name)), name
    for n, width_L in ((0, 59), (3, 5), (12, 2), (12, 1), (1000, 3), (1000, 4), (30, 1)):
        assert interface.demo_texts(n, width_L) == ec.demo_texts(n, width_L), (n, width_L)
    with pytest.raises(ValueError):
        interface.decode_texts([])
