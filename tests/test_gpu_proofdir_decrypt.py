"""GPU suite: the decryption half of the proof directory (verificatum-vmn_amd/proofdir.py: write_decryption, verify_decryption)
at widths 1 and 3 over the 512-bit group, k = 3 parties, threshold 2, N = 30.

The C++ drivers play DistrElGamalSession.decrypt and write proofs/PolynomialInExponent.bt, DecryptionFactors%02d.bt,
DecrFactCommitment%02d.bt, DecrFactReply%02d.bt, CorrectIndices.bt and Plaintexts.bt; the verifier's branch
(MixNetElGamalVerifyFiatShamirSession.java:1545-1667) reads them back.  Dec.s, Dec.v and the public key shares are compared
with values computed by hashlib and the integer restatement (tests/wide_decrypt_ref.py) from the SAME files.

Wall time on an MI355X: not measured yet, for this module and for the existing GPU modules beside it."""
import hashlib
import os

import pytest

from conftest import load_golden
from oracle import pyref, pyref_prg

import wide_decrypt_ref as Wref

pytestmark = pytest.mark.gpu

K, THR, N = 3, 2, 30


def _params(p, q, g, width):
    return {"version": "3.1.0", "sid": "SessionID", "auxsid": "default", "rbitlen": 100, "vbitlenro": 256, "ebitlenro": 256,
            "prg": "SHA-256", "rohash": "SHA-256", "rohash_name": "SHA-256", "width": width, "k": K, "threshold": THR,
            "pgroup": "ModPGroup(512)", "group": {"kind": "modp", "p": format(p, "x"), "q": format(q, "x"), "g": format(g, "x")}}


def _array(buf, pos, eb):
    """(integers, next position) of an array byte tree node(n leaves of eb bytes) at buf[pos:]."""
    assert buf[pos] == 0
    n = int.from_bytes(buf[pos + 1:pos + 5], "big")
    pos += 5
    out = []
    for _ in range(n):
        assert buf[pos:pos + 5] == b"\x01" + eb.to_bytes(4, "big")
        out.append(int.from_bytes(buf[pos + 5:pos + 5 + eb], "big"))
        pos += 5 + eb
    return out, pos


def _wide_array(path, width, eb):
    buf = open(path, "rb").read()
    pos = 0
    if width > 1:
        assert buf[:5] == b"\x00" + width.to_bytes(4, "big")
        pos = 5
    comps = []
    for _ in range(width):
        a, pos = _array(buf, pos, eb)
        comps.append(a)
    assert pos == len(buf)
    return comps


@pytest.fixture(scope="module")
def mods(entry):
    import mirror
    return mirror.load(entry, ("proofdir", "randomsource", "fiatshamir", "native"))


def make(mods, vmn, gpu_ctx, width, nizkp, tamper=None):
    pd, rs = mods["proofdir"], mods["randomsource"]
    grpd, _ = load_golden(512)
    p, q, g = grpd["p"], grpd["q"], grpd["g"]
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    params = _params(p, q, g, width)
    tape = rs.InsecureShaRandomSource(b"proofdir-dec%d" % width, q)
    coeffs = tape.ring_array(THR)
    shares = [None] + [sum(c * pow(l, d, q) for d, c in enumerate(coeffs)) % q for l in range(1, K + 1)]
    poly = [pow(g, c, p) for c in coeffs]
    y = poly[0]
    pkey = [g] * width + [y] * width
    enc = [tape.ring_array(N) for _ in range(width)]
    msgs = [pyref.exp_fixed(g, tape.ring_array(N), p) for _ in range(width)]
    w = [pyref.exp_fixed(g, enc[c], p) for c in range(width)] + [pyref.mul(msgs[c], pyref.exp_fixed(y, enc[c], p), p) for c in range(width)]
    W = [G.toElementArray(c) for c in w]
    pd.write_inputs(nizkp, G, params, pkey, W)
    plain = pd.write_decryption(nizkp, G, params, pkey, W, poly, shares, rs.InsecureShaRandomSource(b"proofdir-dec-prover", q), K, THR,
                                tamper=tamper)
    return dict(G=G, p=p, q=q, g=g, params=params, pkey=pkey, poly=poly, shares=shares, y=y, w=w, msgs=msgs, plain=plain)


@pytest.mark.parametrize("width", [1, 3])
def test_decryption_directory_round_trip_and_test_vectors(width, mods, vmn, gpu_ctx, tmp_path):
    pd, fs = mods["proofdir"], mods["fiatshamir"]
    nizkp = str(tmp_path / "nizkp")
    I = make(mods, vmn, gpu_ctx, width, nizkp)
    G, p, q, g, params, pkey = I["G"], I["p"], I["q"], I["g"], I["params"], I["pkey"]
    eb = G.elem_bytes
    assert [a.toInts() for a in I["plain"]] == I["msgs"]
    tv = {}
    assert pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0), tv)
    # Plaintexts.bt decodes to the messages that were encrypted; CorrectIndices.bt: k + 1 booleans, all set
    assert _wide_array(pd.plaintexts_file(nizkp), width, eb) == I["msgs"]
    assert open(pd.cr_file(nizkp), "rb").read() == b"\x01" + (K + 1).to_bytes(4, "big") + b"\x01" * (K + 1)
    # ---- the same files through hashlib and the integer restatement
    ref = Wref.adapter_modp(p, q)
    poly_bt = open(pd.poly_file(nizkp), "rb").read()
    poly, _ = _array(poly_bt, 0, eb)
    assert poly == I["poly"]
    ys = [None]
    for l in range(1, K + 1):
        yl = 1
        for d, c in enumerate(poly):
            yl = yl * pow(c, l ** d, p) % p
        ys.append(yl)
        assert tv["Dec.y_%d" % l] == format(yl, "x") and yl == pow(g, I["shares"][l], p)
    rho = pd.global_prefix(params)
    list_bytes = open(pd.l_file(nizkp, 0), "rb").read()
    df = [open(pd.df_file(nizkp, l), "rb").read() for l in range(1, K + 1)]
    node = lambda n: b"\x00" + n.to_bytes(4, "big")
    seed_data = node(2) + node(2) + fs.leaf(G.enc_el(g)) + list_bytes + node(2) + poly_bt + node(K) + b"".join(df)
    seed = pyref_prg.random_oracle(rho + seed_data, 8 * hashlib.sha256().digest_size)
    assert tv["Dec.s"] == seed.hex()
    com = [open(pd.dfc_file(nizkp, l), "rb").read() for l in range(1, K + 1)]
    v = int.from_bytes(pyref_prg.random_oracle(rho + node(2) + fs.leaf(seed) + node(K) + b"".join(com), 256), "big")
    assert tv["Dec.v"] == str(v)
    # the restatement accepts the files: per party and combined
    u, vv = I["w"][:width], I["w"][width:]
    f = [None] + [_wide_array(pd.df_file(nizkp, l), width, eb) for l in range(1, K + 1)]
    for l in range(1, K + 1):
        assert f[l] == Wref.decryption_factors(ref, u, I["shares"][l], K)
    o = Wref.WideDistrElGamalSessionBasic(ref, g, 1, K, THR)
    o.setInstance(u, ys, f)
    o.setBatchVector(pyref_prg.random_integers(seed, N, 256))
    o.batchInput()
    for l in range(1, K + 1):
        c = com[l - 1]
        assert c[:5] == node(2) and c[5:10] == b"\x01" + eb.to_bytes(4, "big")
        yp = int.from_bytes(c[10:10 + eb], "big")
        rest = c[10 + eb:]
        if width > 1:
            assert rest[:5] == node(width)
            rest = rest[5:]
        assert len(rest) == width * (5 + eb)
        Bp = tuple(int.from_bytes(rest[i * (5 + eb) + 5:(i + 1) * (5 + eb)], "big") for i in range(width))
        o.setCommitment(l, yp, Bp)
        r = open(pd.dfr_file(nizkp, l), "rb").read()
        assert r[:5] == b"\x01" + G.exp_bytes.to_bytes(4, "big")
        o.setReply(l, int.from_bytes(r[5:], "big"))
        o.batch(l)
        assert o.verify(l, v), l
    correct = [False] + [True] * K
    comb = Wref.combine_decryption_factors(ref, f, correct, K, THR)
    o.combine(correct, I["y"], comb)
    o.batchCombined()
    assert o.verifyCombined(v)
    assert Wref.plaintexts(ref, vv, comb) == I["msgs"]
    # ---- a truncated reply of party 1, a missing file: False, no exception
    path = pd.dfr_file(nizkp, 1)
    good = open(path, "rb").read()
    open(path, "wb").write(good[:-3])
    assert not pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0))
    os.remove(path)
    assert not pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0))
    open(path, "wb").write(good)
    assert pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0))
    # ---- too few correct indices
    crp = pd.cr_file(nizkp)
    good = open(crp, "rb").read()
    open(crp, "wb").write(good[:5] + b"\x00\x01\x00\x00")
    assert not pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0))
    open(crp, "wb").write(good)
    # ---- DecryptionFactors02.bt corrupted (one element of the last component times g: still a group element) while
    # CorrectIndices.bt claims party 2
    path = pd.df_file(nizkp, 2)
    good = open(path, "rb").read()
    el = int.from_bytes(good[-eb:], "big") * g % p
    open(path, "wb").write(good[:-eb] + el.to_bytes(eb, "big"))
    assert not pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0))
    open(path, "wb").write(good)
    assert pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0))


@pytest.mark.parametrize("width", [1, 3])
def test_a_party_with_wrong_factors_is_marked_incorrect_by_the_prover(width, mods, vmn, gpu_ctx, tmp_path):
    """Party 2 publishes factors with one wrong element: the combined proof of the first two parties fails, every party is
    verified on its own, CorrectIndices.bt drops party 2, and parties 1 and 3 decrypt -- the same plaintexts."""
    pd = mods["proofdir"]
    nizkp = str(tmp_path / "nizkp")
    box = {}

    def tamper(l, factors):
        if l != 2:
            return factors
        G = factors[0].group
        last = factors[-1].toInts()
        last[N - 1] = last[N - 1] * G.g % G.p
        box["replaced"] = factors[-1]
        return factors[:-1] + [G.toElementArray(last)]
    I = make(mods, vmn, gpu_ctx, width, nizkp, tamper=tamper)
    G, params, pkey = I["G"], I["params"], I["pkey"]
    assert "replaced" in box
    assert open(pd.cr_file(nizkp), "rb").read() == b"\x01" + (K + 1).to_bytes(4, "big") + bytes([1, 1, 0, 1])
    assert [a.toInts() for a in I["plain"]] == I["msgs"]
    assert _wide_array(pd.plaintexts_file(nizkp), width, G.elem_bytes) == I["msgs"]
    tv = {}
    assert pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0), tv)
    assert tv["Dec.s"] and int(tv["Dec.v"]) > 0
    # the same files with CorrectIndices.bt still claiming party 2: rejected
    open(pd.cr_file(nizkp), "wb").write(b"\x01" + (K + 1).to_bytes(4, "big") + b"\x01" * (K + 1))
    assert not pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0))
