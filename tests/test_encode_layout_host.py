"""CPU suite: the byte-level rules of the message encoding (csrc/encode_layout.h) as host code under AddressSanitizer and UBSan,
through a stand-alone program (tests/encode_layout_harness.cpp) that fills records byte by byte as k_textlines_records does, folds
them as k_textlines_fold does and walks payloads as k_textlines_lengths does.  Over the catalogue of tests/encode_cases.py the
records are the restatement's values on the wire width, the folded records and their lengths are the restatement's decoding --
of v and of p - v, of ill-formed values too -- and the UTF-8 verdicts and stripped bytes are the restatement's."""
import os
import subprocess

import pytest

from conftest import ROOT, load_golden

import encode_cases as ec


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("encode") / "encode_layout_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "encode_layout_harness.cpp")], check=True)
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
    for bits, want in list(ec.ENCODE_LENGTH.items()) + [(41, 0), (42, 1), (49, 1), (50, 2), (34, 0), (2, 0), (1, 0), (0, 0)]:
        r = subprocess.run([harness, "length", str(bits)], capture_output=True, text=True)
        assert r.returncode == 0 and int(r.stdout) == want == (max(0, (bits - 2) // 8 - 4) if bits >= 2 else 0), bits


# the golden groups at the bytes of the modulus, and one at the reference's wider leaf
SHAPES = [(512, 64), (1024, 128), (1024, 129), (2048, 256), (3072, 384), (4096, 512)]


@pytest.mark.parametrize("bits,nbytes", SHAPES)
def test_records_are_the_values_on_the_wire_width(harness, tmp_path, bits, nbytes):
    g, _ = load_golden(bits)
    L = ec.encode_length(g["p"])
    for ncomp in ec.NCOMPS:
        msgs = ec.messages(L, ncomp)
        got = run(harness, tmp_path, msgs, "records", nbytes, L, ncomp)
        for msg, line in zip(msgs, got):
            want = " ".join(ec.value_of(piece, L).to_bytes(nbytes, "big").hex() for piece in ec.pieces(msg, ncomp, L))
            assert line == want, (ncomp, msg[:20])


@pytest.mark.parametrize("bits,nbytes", SHAPES)
def test_the_fold_is_the_restatements_decoding(harness, tmp_path, bits, nbytes):
    g, _ = load_golden(bits)
    p, q = g["p"], g["q"]
    L = ec.encode_length(p)
    tail = ec.stream(b"behind", L - 2)
    values = [ec.value_of(m, L) for m in ec.messages(L, 1) + list(ec.STRIPPED) + list(ec.BAD_UTF8)]
    values += ec.ill_formed_values(p)
    values += [int.from_bytes((2).to_bytes(4, "big") + b"hi" + tail, "big"), (1 << (8 * (L + 4))) - 1, 1 << (8 * (L + 4)), q, q - 1, 1]
    elements = values + [p - v for v in values]
    got = run(harness, tmp_path, [e.to_bytes(nbytes, "big") for e in elements], "fold", nbytes, L, p.to_bytes(nbytes, "big").hex(),
              q.to_bytes(nbytes, "big").hex())
    ill = 0
    for e, line in zip(elements, got):
        msg, ok = ec.decode_element(e, p)
        if not ok:
            assert line == "ill", e
            ill += 1
            continue
        v = min(e, p - e)
        n, T = line.split(" ")
        assert int(n) == len(msg) and bytes.fromhex(T) == v.to_bytes(L + 4, "big") and bytes.fromhex(T)[4:4 + len(msg)] == msg, e
    assert ill >= 2 * (len(ec.ill_formed_values(p)) + 1)


def test_utf8_verdicts_and_stripping(harness, tmp_path):
    samples = list(ec.BAD_UTF8) + list(ec.STRIPPED) + [ec.C3_0A_A9, b"", b"plain", ec.E_ACUTE, ec.EURO, ec.G_CLEF]
    samples += [ec.stream(b"utf8/%d" % k, 1 + k % 9) for k in range(400)] + ec.messages(59, 2)
    samples += [bytes([a, b]) for a in range(0xC0, 0x100) for b in (0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0)]
    samples += [bytes([a, b, 0x80]) for a in range(0xE0, 0xF5) for b in (0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0)]
    samples += [bytes([a, b, 0x80, 0x80]) for a in range(0xF0, 0xF6) for b in (0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0)]
    got = run(harness, tmp_path, samples, "utf8")
    seen = set()
    for s, line in zip(samples, got):
        verdict, kept = (line.split(" ") + [""])[:2]
        try:
            s.decode("utf-8")
            want = True
        except UnicodeDecodeError:
            want = False
        assert (verdict == "1") == want == ec.utf8_wellformed(s), s
        assert bytes.fromhex(kept) == s.replace(b"\n", b"").replace(b"\r", b""), s
        seen.add(want)
    assert seen == {True, False}
