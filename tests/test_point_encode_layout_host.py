"""CPU suite: the byte-level rules of the message encoding over curves (csrc/ec_encode_layout.h) as host code under
AddressSanitizer and UBSan, through a stand-alone program (tests/point_encode_layout_harness.cpp) that fills the records T byte by
byte as k_textlines_records does at nbytes = L + 4 and folds point records as k_ec_textlines_fold does.  Over the catalogue of
tests/point_encode_cases.py the records are floor(x / 256) of the restatement's points, and the folded records and their lengths
are the restatement's decoding -- of (x, y) and (x, p - y), of a second counter, of ill-formed points and of infinity."""
import os
import subprocess

import pytest

from conftest import ROOT

import encode_cases as ec
import point_encode_cases as pe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("point_encode") / "point_encode_layout_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "point_encode_layout_harness.cpp")], check=True)
    return exe


def run(exe, tmp_path, items, *args):
    path = str(tmp_path / "items")
    with open(path, "w") as f:
        f.write("".join(b.hex() + "\n" for b in items))
    r = subprocess.run([exe] + [str(a) for a in args] + [path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(items)
    return lines


def test_the_encode_length(harness):
    for bits, want in list(pe.ENCODE_LENGTH.items()) + [(49, 0), (50, 1), (57, 1), (58, 2), (42, 0), (2, 0), (1, 0), (0, 0)]:
        r = subprocess.run([harness, "length", str(bits)], capture_output=True, text=True)
        assert r.returncode == 0 and int(r.stdout) == want == (max(0, (bits - 2) // 8 - 5) if bits >= 2 else 0), bits


# (curve, bytes of a coordinate): the natural width, and P-256 at the reference's wider leaf
SHAPES = [("P-192", 24), ("P-224", 28), ("prime239v1", 30), ("P-256", 32), ("P-256", 33), ("secp256k1", 32), ("P-384", 48),
          ("brainpoolp512r1", 64), ("P-521", 66)]


@pytest.mark.parametrize("name,nbytes", SHAPES)
def test_records_are_the_x_coordinates_without_their_counter(harness, tmp_path, name, nbytes):
    L = pe.encode_length(pe.curve(name)["p"])
    for ncomp in pe.NCOMPS:
        msgs = pe.messages(name, ncomp)
        got = run(harness, tmp_path, msgs, "records", L, ncomp)
        for msg, line in zip(msgs, got):
            want = " ".join((P[0] // 256).to_bytes(L + 4, "big").hex() for P in pe.encode_message(msg, name, ncomp))
            assert line == want, (ncomp, msg[:20])


@pytest.mark.parametrize("name,nbytes", SHAPES)
def test_the_fold_is_the_restatements_decoding(harness, tmp_path, name, nbytes):
    cv = pe.curve(name)
    L = pe.encode_length(cv["p"])
    points = [pe.encode_piece(m, name)[0] for m in pe.messages(name, 1) + list(ec.STRIPPED) + list(ec.BAD_UTF8) + [ec.C3_0A_A9]]
    points += [pe.other_counter(b"twice", name), pe.encode_piece(b"twice", name)[0]]
    points += pe.ill_formed_points(name)
    points += [pe.craft(name, L, b"point-encode/full"), pe.craft(name, 0, b"point-encode/behind")]      # bytes behind the message are ignored
    points += [pe.negated(P, name) for P in points]
    # rows that are no points at all still fold by the rule: the largest x below the bound, and the bound itself
    raw = [pe.point_bytes(P, nbytes) for P in points]
    raw += [v.to_bytes(nbytes, "big") + b"\x00" * nbytes for v in ((1 << (8 * (L + 5))) - 1, 1 << (8 * (L + 5)))]
    raw += [b"\xff" * nbytes + b"\xff" * (nbytes - 1) + b"\xfe"]                                         # not quite infinity
    got = run(harness, tmp_path, raw, "fold", nbytes, L)
    ill = 0
    for rec, line in zip(raw, got):
        x = int.from_bytes(rec[:nbytes], "big")
        msg, ok = pe.decode_point(None if rec == b"\xff" * (2 * nbytes) else (x, 0), name)
        if not ok:
            assert line == "ill", rec.hex()
            ill += 1
            continue
        n, T = line.split(" ")
        assert int(n) == len(msg) and bytes.fromhex(T) == (x // 256).to_bytes(L + 4, "big") and bytes.fromhex(T)[4:4 + len(msg)] == msg, rec.hex()
    assert ill >= 2 * len(pe.ill_formed_points(name)) + 3
