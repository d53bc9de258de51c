"""CPU suite: what the json interface does on the host -- the argument handling of tools/vmnc_convert.py (json is an interface
of -ini and -outi, -plain writes json or raw, a curve group with json is a usage error) and the public key file of
verificatum_vmn_amd/interface.py (ProtocolElGamalInterfaceJSON.java:110-126, 151-206): a round trip, a missing key, the default
encoding, y outside the group.  No GPU: the tool is driven only as far as its arguments and its input file."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden


def run_tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vmnc_convert.py")] + list(args), capture_output=True, text=True,
                          timeout=120)


def test_the_tool_takes_json_and_refuses_it_over_a_curve(entry, tmp_path):
    missing, out = str(tmp_path / "missing"), str(tmp_path / "out")
    for ini, outi in (("json", "raw"), ("raw", "json"), ("native", "json"), ("json", "native"), ("json", "json")):
        r = run_tool("-ciphs", "-ini", ini, "-outi", outi, "--bits", "2048", missing, out)
        assert r.returncode == 1 and "no such file" in r.stderr, (ini, outi, r.returncode, r.stderr[-1000:])     # past the arguments
        r = run_tool("-ciphs", "-ini", ini, "-outi", outi, "--curve", "P-256", missing, out)
        assert r.returncode == 2 and "modular groups only" in r.stderr, (ini, outi, r.returncode, r.stderr[-1000:])
    for outi in ("json", "raw"):
        r = run_tool("-plain", "-outi", outi, "-width", "3", "--bits", "2048", missing, out)
        assert r.returncode == 1 and "no such file" in r.stderr, (outi, r.returncode, r.stderr[-1000:])
    assert run_tool("-plain", "-outi", "json", "--curve", "P-256", missing, out).returncode == 2
    assert run_tool("-plain", "-outi", "native", "--bits", "2048", missing, out).returncode == 2
    assert run_tool("-plain", "-ini", "raw", "-outi", "json", "--bits", "2048", missing, out).returncode == 2
    assert run_tool("-ciphs", "-outi", "json", "--bits", "2048", missing, out).returncode == 2          # -ciphs needs -ini
    assert run_tool("-ciphs", "-plain", "-ini", "json", "-outi", "raw", "--bits", "2048", missing, out).returncode == 2
    assert run_tool("-ciphs", "-ini", "json", "-outi", "xml", "--bits", "2048", missing, out).returncode == 2
    assert run_tool("-ciphs", "-ini", "native", "-outi", "raw", "--curve", "P-256", missing, out).returncode == 1     # curves keep native and raw
    assert not os.path.exists(out)


@pytest.fixture(scope="module")
def interface(vmn):
    from verificatum_vmn_amd import interface
    return interface


def test_public_key_file(interface, tmp_path):
    g, _ = load_golden(512)
    p, q, gen = g["p"], g["q"], g["g"]
    assert p == 2 * q + 1
    y = pow(gen, 0x1234567, p)
    path = str(tmp_path / "pk.json")
    interface.write_public_key_json(path, p, q, gen, y)
    text = open(path).read()
    assert text == '{"g":"%d","p":"%d","q":"%d","y":"%d","encoding":"1"}' % (gen, p, q, y)           # the reference's order, no spaces
    assert interface.read_public_key_json(path) == {"p": p, "q": q, "g": gen, "y": y, "encoding": 1}
    interface.write_public_key_json(path, p, q, gen, y, encoding=2)
    assert interface.read_public_key_json(path)["encoding"] == 2
    # at least p, q, g and y
    full = {"g": str(gen), "p": str(p), "q": str(q), "y": str(y)}
    for key in full:
        open(path, "w").write(json.dumps({k: v for k, v in full.items() if k != key}))
        with pytest.raises(ValueError, match=key + " missing"):
            interface.read_public_key_json(path)
    # without "encoding": 1 for a safe prime, else 2
    open(path, "w").write(json.dumps(full))
    assert interface.read_public_key_json(path)["encoding"] == 1
    sub_p, sub_q = 607, 101                                           # 607 = 6 * 101 + 1: a subgroup of a prime that is not safe
    sub_g = pow(3, (sub_p - 1) // sub_q, sub_p)
    assert sub_g != 1
    open(path, "w").write(json.dumps({"p": str(sub_p), "q": str(sub_q), "g": str(sub_g), "y": str(pow(sub_g, 5, sub_p))}))
    assert interface.read_public_key_json(path) == {"p": sub_p, "q": sub_q, "g": sub_g, "y": pow(sub_g, 5, sub_p), "encoding": 2}
    interface.write_public_key_json(path, sub_p, sub_q, sub_g, pow(sub_g, 5, sub_p))
    assert '"encoding":"2"' in open(path).read()
    # y must lie in the group: a non-residue, zero, p, a number that is no decimal string
    for bad in (p - y, 0, p, p + y):
        open(path, "w").write(json.dumps(dict(full, y=str(bad))))
        with pytest.raises(ValueError, match="y is not in the group"):
            interface.read_public_key_json(path)
    for bad in ("-1", "0x10", "", " 5", 5):
        open(path, "w").write(json.dumps(dict(full, y=bad)))
        with pytest.raises(ValueError):
            interface.read_public_key_json(path)
    for text in ("", "[]", '"x"', "{"):
        open(path, "w").write(text)
        with pytest.raises(ValueError):
            interface.read_public_key_json(path)
