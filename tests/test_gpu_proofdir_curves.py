"""GPU suite: proof directories over curve groups (verificatum-vmn_amd/proofdir.py, tools/vmnv_vectors.py --curve).

The same files as over a modular group (tests/test_gpu_proofdir.py, tests/test_gpu_proofdir_decrypt.py), with a group element
written and hashed as node(leaf(x), leaf(y)) of the group's coordinate wire width (33 bytes for P-256 and secp256k1, 66 for
P-521 at the reference's widths), the point at infinity as (-1, -1), and an array of n points taking 5 + n (15 + 2 cw) bytes.
That shape of a point and of an array of points is this library's existing wire format (what the array export and the C++
message container write); it is pinned by these tests and tests/ec_wire_edges.py, not by a run of the reference.

Seeds, challenges and der.rho are recomputed here from the files' bytes with a parser and an encoder of this module's own and
hashlib (through oracle/pyref_prg.py's random oracle); the verifiers' intermediates come from the affine-point oracle
(oracle/pyref_ec.py under oracle/pyref_proofs.py's GPoS / GCCPoS), the decryption from tests/wide_decrypt_ref.py.

Wall time of each test on an MI355X (one run, pytest's call durations): PoS over P-256 1.7 s; PoS over secp256k1 0.04 s and
over P-521 0.2 s; the precomputed shuffle 0.7 s; the decryption 1.0 s at width 1 and 0.4 s at width 3; a party with wrong
factors 0.04 s and 0.07 s; the tool 0.4 s; the module 5.7 s with its set-up."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from oracle import pyref_ec, pyref_prg, pyref_proofs as P

import wide_decrypt_ref as Wref

pytestmark = pytest.mark.gpu

NV = NE = 256
NR = 100


# ---- this module's own byte-tree encoder / parser -----------------------------------------------------------------------
def node(n):
    return b"\x00" + n.to_bytes(4, "big")


def leaf(data):
    return b"\x01" + len(data).to_bytes(4, "big") + data


def point_node(pt, cw):
    if pt is None:
        return node(2) + leaf(b"\xff" * cw) * 2
    return node(2) + leaf(pt[0].to_bytes(cw, "big")) + leaf(pt[1].to_bytes(cw, "big"))


def array_node(pts, cw):
    return node(len(pts)) + b"".join(point_node(pt, cw) for pt in pts)


def key_node(pkey, cw):
    half = len(pkey) // 2
    enc = [point_node(pt, cw) for pt in pkey]
    if half == 1:
        return node(2) + enc[0] + enc[1]
    return node(2) + node(half) + b"".join(enc[:half]) + node(half) + b"".join(enc[half:])


def parse(buf, pos=0):
    """(tree, next position): a leaf is its bytes, a node the list of its children."""
    assert len(buf) >= pos + 5 and buf[pos] in (0, 1)
    count = int.from_bytes(buf[pos + 1:pos + 5], "big")
    if buf[pos] == 1:
        assert len(buf) >= pos + 5 + count
        return bytes(buf[pos + 5:pos + 5 + count]), pos + 5 + count
    pos += 5
    out = []
    for _ in range(count):
        child, pos = parse(buf, pos)
        out.append(child)
    return out, pos


def tree_of(path):
    buf = open(path, "rb").read()
    t, end = parse(buf)
    assert end == len(buf)
    return t


def pt(t, cw):
    """The point of a parsed point node: two leaves of cw bytes; (-1, -1) is infinity."""
    assert isinstance(t, list) and len(t) == 2 and all(isinstance(c, bytes) and len(c) == cw for c in t)
    if t[0] == t[1] == b"\xff" * cw:
        return None
    return int.from_bytes(t[0], "big"), int.from_bytes(t[1], "big")


def pts(t, cw):
    return [pt(x, cw) for x in t]


def num(t):
    assert isinstance(t, bytes)
    return int.from_bytes(t, "big")


def hexpt(x):
    return "INFINITY" if x is None else "(%x, %x)" % x


def hexpts(xs):
    return "(" + ", ".join(hexpt(x) for x in xs) + ")"


def own_rho(params):
    s = lambda x: leaf(x.encode("utf-8"))
    i = lambda x: leaf(int(x).to_bytes(4, "big"))
    parts = [s(params["version"]), s(params["sid"] + "." + params["auxsid"]), i(params["rbitlen"]), i(params["vbitlenro"]),
             i(params["ebitlenro"]), s(params["prg"]), s(params["pgroup"]), s(params["rohash"])]
    return hashlib.sha256(node(8) + b"".join(parts)).digest()


def ro(rho, data, bits=256):
    return pyref_prg.random_oracle(rho + data, bits)


def _params(name, width=1, **more):
    out = {"version": "3.1.0", "sid": "SessionID", "auxsid": "default", "rbitlen": NR, "vbitlenro": NV, "ebitlenro": NE,
           "prg": "SHA-256", "rohash": "SHA-256", "rohash_name": "SHA-256", "width": width,
           "pgroup": f"ECqPGroup({name})", "group": {"kind": "ec", "curve": name}}
    out.update(more)
    return out


def flip(path, index, mask=1):
    good = open(path, "rb").read()
    bad = bytearray(good)
    bad[index] ^= mask
    open(path, "wb").write(bytes(bad))
    return good


@pytest.fixture(scope="module")
def mods(entry):
    import mirror
    return mirror.load(entry, ("proofdir", "randomsource", "fiatshamir", "native"))


@pytest.fixture(scope="module")
def p256(vmn, gpu_ctx):
    G = vmn.ECqPGroup(gpu_ctx, "P-256", java_widths=True)
    assert G.nbytes == 33 and G.coord_bytes == 33
    return G, pyref_ec.Curve("P-256")


def gpu_list(G, tape, y, n, width):
    """A list of n ciphertexts of `width` under the key y, made on the GPU: (device arrays, points, message points)."""
    T = [G.ringArray(tape.ring_array(n)) for _ in range(width)]
    M = [G.exp(G.g, G.ringArray(tape.ring_array(n))) for _ in range(width)]
    W = [G.exp(G.g, t) for t in T] + [m.mul(G.exp(y, t)) for m, t in zip(M, T)]
    return W, [a.toInts() for a in W], [m.toInts() for m in M]


# ---- (a) PoS, P-256, width 1, n = 40, with (infinity, infinity) among the inputs ------------------------------------------
def test_pos_directory_over_p256_round_trip_and_test_vectors(mods, p256, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    G, c = p256
    cw, n, INF_AT = 33, 40, 7
    params = _params("P-256")
    tape = rs.InsecureShaRandomSource(b"proofdir-ec", c.n)
    y = c.mul(tape.ring_element(), c.g)
    pkey = [c.g, y]
    t_enc, msgs = tape.ring_array(n), tape.ring_array(n)
    w = [c.exp_fixed(c.g, t_enc), c.mul_arrays(c.exp_fixed(c.g, msgs), c.exp_fixed(y, t_enc))]
    w[0][INF_AT] = w[1][INF_AT] = None
    W = [G.toElementArray(col) for col in w]
    nizkp = str(tmp_path / "nizkp")
    pd.write_inputs(nizkp, G, params, pkey, W)
    WP = pd.write_shuffle(nizkp, 1, G, params, pkey, W, rs.InsecureShaRandomSource(b"proofdir-ec-prover", c.n))
    tv = {}
    assert pd.verify_shuffle(nizkp, 1, G, params, pkey, tv, with_arrays=True)
    assert tv["verdicts(A,B,C,D,F)"] == str((True,) * 5)

    # ---- the files: sizes and contents, through this module's parser
    list_size = 5 + 2 * (5 + n * (15 + 2 * cw))
    assert os.path.getsize(pd.l_file(nizkp, 0)) == os.path.getsize(pd.l_file(nizkp, 1)) == list_size
    assert open(pd.pk_file(nizkp), "rb").read() == key_node(pkey, cw)
    l0, l1 = open(pd.l_file(nizkp, 0), "rb").read(), open(pd.l_file(nizkp, 1), "rb").read()
    assert l0 == node(2) + array_node(w[0], cw) + array_node(w[1], cw)
    assert node(2) + leaf(b"\xff" * cw) * 2 in l0                               # the (-1, -1) encoding went through the list file
    w_files = [pts(col, cw) for col in tree_of(pd.l_file(nizkp, 0))]
    assert w_files == w and w_files[0][INF_AT] is None and w_files[1][INF_AT] is None
    wp = [pts(col, cw) for col in tree_of(pd.l_file(nizkp, 1))]
    assert wp == [a.toInts() for a in WP]
    u_bt = open(pd.pc_file(nizkp, 1), "rb").read()
    u = pts(tree_of(pd.pc_file(nizkp, 1)), cw)
    assert len(u) == n and len(u_bt) == 5 + n * (15 + 2 * cw)

    # ---- der.rho, bas.h, PoS.s, PoS.v from the files' bytes
    rho = own_rho(params)
    assert tv["der.rho"] == rho.hex()
    h = pyref_prg.ec_generators(ro(rho, leaf(b"generators")), n, c, NR)
    assert tv["bas.h"] == hexpts(h)
    inst = node(6) + point_node(c.g, cw) + array_node(h, cw) + u_bt + key_node(pkey, cw) + l0 + l1
    seed = ro(rho, inst)
    assert tv["PoS.s"] == seed.hex()
    com_bt = open(pd.posc_file(nizkp, 1), "rb").read()
    v = int.from_bytes(ro(rho, node(2) + leaf(seed) + com_bt, NV), "big")
    assert tv["PoS.v"] == format(v, "x")

    # ---- the oracle's verifier on the parsed messages
    ct = tree_of(pd.posc_file(nizkp, 1))
    assert len(ct) == 6
    com_o = {"B": pts(ct[0], cw), "Ap": pt(ct[1], cw), "Bp": pts(ct[2], cw), "Cp": pt(ct[3], cw), "Dp": pt(ct[4], cw),
             "Fp": pts(ct[5], cw)}
    rt = tree_of(pd.posr_file(nizkp, 1))
    assert len(rt) == 6
    rep_o = {"k_A": num(rt[0]), "k_B": [num(x) for x in rt[1]], "k_C": num(rt[2]), "k_D": num(rt[3]),
             "k_E": [num(x) for x in rt[4]], "k_F": [num(rt[5])]}
    assert len(com_o["B"]) == len(com_o["Bp"]) == len(rep_o["k_B"]) == len(rep_o["k_E"]) == n and len(com_o["Fp"]) == 2
    ov = P.GPoS(P.ECAdapter(c), NV, NE, NR)
    ov.precompute(c.g, h)
    ov.u = u
    ov.setInstance(pkey, w_files, wp)
    ov.setBatchVector(pyref_prg.random_integers(seed, n, NE))
    ov.computeAF()
    ov.setCommitment(com_o)
    assert ov.verify(rep_o, v)
    assert (tv["PoS.A"], tv["PoS.C"], tv["PoS.D"]) == (hexpt(ov.A), hexpt(ov.C), hexpt(ov.D))
    assert tv["PoS.F"] == hexpts(ov.F)
    assert tv["PoS.k_A"] == format(rep_o["k_A"], "x") and tv["PoS.Ap"] == hexpt(com_o["Ap"])

    # ---- tampering: False without an exception, then restored and accepted
    verify = lambda: pd.verify_shuffle(nizkp, 1, G, params, pkey)
    path = pd.posr_file(nizkp, 1)
    good = flip(path, -1)                                                       # the last bit of the reply
    assert not verify()
    open(path, "wb").write(good[:-3])                                           # a truncated reply
    assert not verify()
    open(path, "wb").write(good)
    path = pd.l_file(nizkp, 1)
    el = 5 + 5 + 3 * (15 + 2 * cw)                                              # element 3 of the first component array
    assert l1[el:el + 10] == node(2) + b"\x01" + cw.to_bytes(4, "big")
    good = flip(path, el + 15 + 2 * cw - 1)                                     # low bit of its y: off the curve
    assert not verify()
    open(path, "wb").write(good)
    bad = bytearray(good)
    bad[el + 6:el + 10] = (cw - 1).to_bytes(4, "big")                           # its x leaf claims one byte less
    open(path, "wb").write(bytes(bad))
    assert not verify()
    open(path, "wb").write(good)
    assert verify()


# ---- (b) the same round trip over a general-a curve and over the widest coordinate ----------------------------------------
@pytest.mark.parametrize("name, cw", [("secp256k1", 33), ("P-521", 66)])
def test_pos_directory_over_other_curves(name, cw, mods, vmn, gpu_ctx, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    G = vmn.ECqPGroup(gpu_ctx, name, java_widths=True)
    assert G.nbytes == cw
    n = 24
    params = _params(name)
    tape = rs.InsecureShaRandomSource(b"proofdir-ec-" + name.encode(), G.q)
    y = G.k_exp(G.g, tape.ring_element())
    pkey = [G.g, y]
    W, w, _ = gpu_list(G, tape, y, n, 1)
    nizkp = str(tmp_path / "nizkp")
    pd.write_inputs(nizkp, G, params, pkey, W)
    pd.write_shuffle(nizkp, 1, G, params, pkey, W, rs.InsecureShaRandomSource(b"proofdir-ec-prover", G.q))
    assert open(pd.l_file(nizkp, 0), "rb").read() == node(2) + array_node(w[0], cw) + array_node(w[1], cw)
    assert os.path.getsize(pd.l_file(nizkp, 1)) == 5 + 2 * (5 + n * (15 + 2 * cw))
    assert os.path.getsize(pd.pc_file(nizkp, 1)) == 5 + n * (15 + 2 * cw)
    tv = {}
    assert pd.verify_shuffle(nizkp, 1, G, params, pkey, tv)
    assert tv["der.rho"] == own_rho(params).hex()
    good = flip(pd.posr_file(nizkp, 1), -1)
    assert not pd.verify_shuffle(nizkp, 1, G, params, pkey)
    open(pd.posr_file(nizkp, 1), "wb").write(good)
    assert pd.verify_shuffle(nizkp, 1, G, params, pkey)


# ---- (c) the precomputed shuffle, P-256, width 3 ---------------------------------------------------------------------------
def test_precomputed_shuffle_directory_over_p256_width_3(mods, p256, tmp_path):
    """PoSC for N_0 = 40, keep list, CCPoS for the n = 30 ciphertexts that arrived.  The directory's verifier is the standalone
    one (the plain two-equation CCPoS form); the raised single-equation form is what a mix server checks online with u^rho and
    h^rho, so it is run here on the SAME files through the C++ driver."""
    pd, rs, nat = mods["proofdir"], mods["randomsource"], mods["native"]
    G, c = p256
    cw, n_max, n, width = 33, 40, 30, 3
    params = _params("P-256", width)
    tape = rs.InsecureShaRandomSource(b"proofdir-ec-cc", c.n)
    y = G.k_exp(G.g, tape.ring_element())
    pkey = [c.g] * width + [y] * width
    W, w, _ = gpu_list(G, tape, y, n, width)
    nizkp = str(tmp_path / "nizkp")
    pd.write_inputs(nizkp, G, params, pkey, W)
    prover_rand = rs.InsecureShaRandomSource(b"proofdir-ec-cc-prover", c.n)
    pi, R, U, H = pd.write_precomputation(nizkp, 1, G, params, n_max, prover_rand)
    WP = pd.write_committed_shuffle(nizkp, 1, G, params, pkey, W, prover_rand, pi, R, U, H)
    tv = {}
    assert pd.verify_precomputed_shuffle(nizkp, 1, G, params, pkey, n_max, tv)

    # ---- seeds and challenges from the files' bytes
    rho = own_rho(params)
    assert tv["der.rho"] == rho.hex()
    h = pyref_prg.ec_generators(ro(rho, leaf(b"generators")), n_max, c, NR)
    assert H.toInts() == h
    u_bt = open(pd.pc_file(nizkp, 1), "rb").read()
    u = pts(tree_of(pd.pc_file(nizkp, 1)), cw)
    assert len(u) == n_max
    s1 = ro(rho, node(3) + point_node(c.g, cw) + array_node(h, cw) + u_bt)
    assert tv["PoSC.s"] == s1.hex()
    v1 = int.from_bytes(ro(rho, node(2) + leaf(s1) + open(pd.poscc_file(nizkp, 1), "rb").read(), NV), "big")
    assert tv["PoSC.v"] == format(v1, "x")
    kl = open(pd.kl_file(nizkp, 1), "rb").read()
    assert kl[:5] == b"\x01" + n_max.to_bytes(4, "big") and len(kl) == 5 + n_max
    keep = [b == 1 for b in kl[5:]]
    assert sum(keep) == n
    u_s = [x for x, k in zip(u, keep) if k]
    l0, l1 = open(pd.l_file(nizkp, 0), "rb").read(), open(pd.l_file(nizkp, 1), "rb").read()
    assert len(l0) == len(l1) == 5 + 2 * (5 + width * (5 + n * (15 + 2 * cw)))
    halves = tree_of(pd.l_file(nizkp, 1))
    wp = [pts(col, cw) for half in halves for col in half]
    assert wp == [a.toInts() for a in WP]
    assert open(pd.pk_file(nizkp), "rb").read() == key_node(pkey, cw)
    inst = node(6) + point_node(c.g, cw) + array_node(h[:n], cw) + array_node(u_s, cw) + key_node(pkey, cw) + l0 + l1
    s2 = ro(rho, inst)
    assert tv["CCPoS.s"] == s2.hex()
    cc_bt = open(pd.ccposc_file(nizkp, 1), "rb").read()
    v2 = int.from_bytes(ro(rho, node(2) + leaf(s2) + cc_bt, NV), "big")
    assert tv["CCPoS.v"] == format(v2, "x")

    # ---- CCPoS.A, CCPoS.B from the affine-point oracle
    oc = P.GCCPoS(P.ECAdapter(c), NV, NE, NR)
    oc.setInstance(c.g, h[:n], u_s, pkey, w, wp)
    oc.setBatchVector(pyref_prg.random_integers(s2, n, NE))
    oc.computeAB()
    assert tv["CCPoS.A"] == hexpt(oc.A) and tv["CCPoS.B"] == hexpts(oc.B)

    # ---- the raised form on the same files
    rho_exp = tape.int_array(1, 50)[0] | 1
    U_s, H_s = U.extract(keep), H.copyOfRange(0, n)
    RU, RH = U_s.exp(rho_exp), H_s.exp(rho_exp)
    com = nat.Message.fromByteTree(G, cc_bt, nat.CCPoSBasicW._com_kinds, [1, 2 * width])
    rep_bt = open(pd.ccposr_file(nizkp, 1), "rb").read()
    rep = nat.Message.fromByteTree(G, rep_bt, nat.CCPoSBasicW._rep_kinds, [1, width, n])
    assert com is not None and rep is not None
    for tamper in (False, True):
        cv = nat.CCPoSBasicW(G, NV, NE, NR)
        cv.setInstance(c.g, H_s, U_s, pkey, W, WP)
        cv.setBatchVectorSeed(s2)
        cv.setCommitment(com)
        cv.computeAB(RU)
        cv.setChallenge(v2 if not tamper else v2 ^ 1)
        assert cv.verify(rep, RH, rho_exp) is (not tamper)
        cv.free()

    # ---- tampering: one more flag in the keep list, a flipped bit in the CCPoS reply
    verify = lambda: pd.verify_precomputed_shuffle(nizkp, 1, G, params, pkey, n_max)
    good = flip(pd.kl_file(nizkp, 1), 5 + keep.index(False))
    assert not verify()
    open(pd.kl_file(nizkp, 1), "wb").write(good)
    good = flip(pd.ccposr_file(nizkp, 1), -1)
    assert not verify()
    open(pd.ccposr_file(nizkp, 1), "wb").write(good)
    assert verify()


# ---- (d) decryption, P-256, widths 1 and 3, k = 3, threshold 2, N = 30 -----------------------------------------------------
K_PARTIES, THR, N_DEC = 3, 2, 30


def make_decryption(mods, p256, width, nizkp, tamper=None):
    pd, rs = mods["proofdir"], mods["randomsource"]
    G, c = p256
    params = _params("P-256", width, k=K_PARTIES, threshold=THR)
    tape = rs.InsecureShaRandomSource(b"proofdir-ec-dec%d" % width, c.n)
    coeffs = tape.ring_array(THR)
    shares = [None] + [sum(a * pow(l, d, c.n) for d, a in enumerate(coeffs)) % c.n for l in range(1, K_PARTIES + 1)]
    poly = [c.mul(a, c.g) for a in coeffs]
    y = poly[0]
    pkey = [c.g] * width + [y] * width
    W, w, msgs = gpu_list(G, tape, y, N_DEC, width)
    pd.write_inputs(nizkp, G, params, pkey, W)
    plain = pd.write_decryption(nizkp, G, params, pkey, W, poly, shares, rs.InsecureShaRandomSource(b"proofdir-ec-dec-prover", c.n),
                                K_PARTIES, THR, tamper=tamper)
    return dict(params=params, pkey=pkey, poly=poly, shares=shares, y=y, w=w, msgs=msgs, plain=plain)


def wide_points(path, width, cw):
    t = tree_of(path)
    return [pts(col, cw) for col in t] if width > 1 else [pts(t, cw)]


@pytest.mark.parametrize("width", [1, 3])
def test_decryption_directory_over_p256(width, mods, p256, tmp_path):
    pd = mods["proofdir"]
    G, c = p256
    cw, k = 33, K_PARTIES
    nizkp = str(tmp_path / "nizkp")
    I = make_decryption(mods, p256, width, nizkp)
    params, pkey = I["params"], I["pkey"]
    assert [a.toInts() for a in I["plain"]] == I["msgs"]
    tv = {}
    verify = lambda vectors=None: pd.verify_decryption(nizkp, G, params, pkey, pd.l_file(nizkp, 0), vectors)
    assert verify(tv)
    assert wide_points(pd.plaintexts_file(nizkp), width, cw) == I["msgs"]
    assert open(pd.cr_file(nizkp), "rb").read() == b"\x01" + (k + 1).to_bytes(4, "big") + b"\x01" * (k + 1)
    poly_bt = open(pd.poly_file(nizkp), "rb").read()
    poly = pts(tree_of(pd.poly_file(nizkp)), cw)
    assert poly == I["poly"] and poly_bt == array_node(I["poly"], cw)
    ys = [None]
    for l in range(1, k + 1):
        yl = None
        for d, coeff in enumerate(poly):
            yl = c.add(yl, c.mul(l ** d, coeff))
        ys.append(yl)
        assert tv["Dec.y_%d" % l] == hexpt(yl) and yl == c.mul(I["shares"][l], c.g)
    # ---- Dec.s, Dec.v from the files' bytes
    rho = own_rho(params)
    list_bytes = open(pd.l_file(nizkp, 0), "rb").read()
    df = [open(pd.df_file(nizkp, l), "rb").read() for l in range(1, k + 1)]
    assert all(len(x) == (5 if width > 1 else 0) + width * (5 + N_DEC * (15 + 2 * cw)) for x in df)
    seed = ro(rho, node(2) + node(2) + point_node(c.g, cw) + list_bytes + node(2) + poly_bt + node(k) + b"".join(df))
    assert tv["Dec.s"] == seed.hex()
    com = [open(pd.dfc_file(nizkp, l), "rb").read() for l in range(1, k + 1)]
    v = int.from_bytes(ro(rho, node(2) + leaf(seed) + node(k) + b"".join(com), NV), "big")
    assert tv["Dec.v"] == str(v)
    # ---- the restatement over affine points: party 1's factors at both widths; at width 1 the whole session and the plaintexts
    ref = Wref.adapter_curve(c)
    u, vv = I["w"][:width], I["w"][width:]
    f = [None] + [wide_points(pd.df_file(nizkp, l), width, cw) for l in range(1, k + 1)]
    assert f[1] == Wref.decryption_factors(ref, u, I["shares"][1], k)
    commitments = []
    for l in range(1, k + 1):
        t = tree_of(pd.dfc_file(nizkp, l))
        assert len(t) == 2
        Bp = tuple(pts(t[1], cw)) if width > 1 else (pt(t[1], cw),)
        assert len(Bp) == width
        commitments.append((pt(t[0], cw), Bp))
        assert com[l - 1] == node(2) + point_node(commitments[-1][0], cw) + (node(width) if width > 1 else b"") + \
            b"".join(point_node(b, cw) for b in Bp)
        r = open(pd.dfr_file(nizkp, l), "rb").read()
        assert r[:5] == b"\x01" + G.exp_bytes.to_bytes(4, "big") and len(r) == 5 + G.exp_bytes
    if width == 1:
        for l in (2, 3):
            assert f[l] == Wref.decryption_factors(ref, u, I["shares"][l], k)
        o = Wref.WideDistrElGamalSessionBasic(ref, c.g, 1, k, THR)
        o.setInstance(u, ys, f)
        o.setBatchVector(pyref_prg.random_integers(seed, N_DEC, NE))
        o.batchInput()
        for l in range(1, k + 1):
            o.setCommitment(l, *commitments[l - 1])
            o.setReply(l, int.from_bytes(open(pd.dfr_file(nizkp, l), "rb").read()[5:], "big"))
            o.batch(l)
            assert o.verify(l, v), l
        correct = [False] + [True] * k
        comb = Wref.combine_decryption_factors(ref, f, correct, k, THR)
        o.combine(correct, I["y"], comb)
        o.batchCombined()
        assert o.verifyCombined(v)
        assert Wref.plaintexts(ref, vv, comb) == I["msgs"]
    # ---- a flipped bit in a reply, a commitment whose leaf has the wrong width, a commitment point off the curve, a missing file
    path = pd.dfr_file(nizkp, 2)
    good = flip(path, -1)
    assert not verify()
    open(path, "wb").write(good)
    path = pd.dfc_file(nizkp, 1)
    good = open(path, "rb").read()
    bad = bytearray(good)
    bad[5 + 5 + 1:5 + 5 + 5] = (cw - 1).to_bytes(4, "big")                      # y'_1: the x leaf claims one byte less
    open(path, "wb").write(bytes(bad))
    assert not verify()
    flip_at = 5 + 15 + 2 * cw - 1                                               # y'_1: low bit of y, off the curve
    bad = bytearray(good)
    bad[flip_at] ^= 1
    open(path, "wb").write(bytes(bad))
    assert not verify()
    open(path, "wb").write(good + b"\x00")                                      # a byte too many
    assert not verify()
    os.remove(path)
    assert not verify()
    open(path, "wb").write(good)
    assert verify()


@pytest.mark.parametrize("width", [1, 3])
def test_a_party_with_wrong_factors_is_marked_incorrect_over_p256(width, mods, p256, tmp_path):
    pd = mods["proofdir"]
    G, c = p256
    k = K_PARTIES
    nizkp = str(tmp_path / "nizkp")
    box = {}

    def tamper(l, factors):
        if l != 2:
            return factors
        last = factors[-1].toInts()
        last[N_DEC - 1] = c.add(last[N_DEC - 1], c.g)
        box["replaced"] = factors[-1]
        return factors[:-1] + [G.toElementArray(last)]
    I = make_decryption(mods, p256, width, nizkp, tamper=tamper)
    assert "replaced" in box
    assert open(pd.cr_file(nizkp), "rb").read() == b"\x01" + (k + 1).to_bytes(4, "big") + bytes([1, 1, 0, 1])
    assert [a.toInts() for a in I["plain"]] == I["msgs"]
    assert wide_points(pd.plaintexts_file(nizkp), width, 33) == I["msgs"]
    tv = {}
    assert pd.verify_decryption(nizkp, G, I["params"], I["pkey"], pd.l_file(nizkp, 0), tv)
    assert tv["Dec.s"] and int(tv["Dec.v"]) > 0
    # the same files with CorrectIndices.bt still claiming party 2: rejected
    open(pd.cr_file(nizkp), "wb").write(b"\x01" + (k + 1).to_bytes(4, "big") + b"\x01" * (k + 1))
    assert not pd.verify_decryption(nizkp, G, I["params"], I["pkey"], pd.l_file(nizkp, 0))


# ---- (e) the tool ------------------------------------------------------------------------------------------------------------
def test_vmnv_vectors_tool_over_a_curve(entry, tmp_path):
    nizkp = str(tmp_path / "demo_ec")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vmnv_vectors.py"), "--demo", nizkp, "--curve", "P-256", "-n", "40",
                          "-t", "der.rho,PoS"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert "\nTEST VECTOR\nder.rho - Derived prefix bytes to all random oracle queries.\n" in text
    for name in ("PoS.s", "PoS.A", "PoS.F", "PoS.Ap", "PoS.v", "PoS.C", "PoS.D", "PoS.k_A", "PoS.k_F"):
        assert f"\nTEST VECTOR\n{name} - " in text, name
    assert "PoS.k_E" not in text
    assert "accepted" in text
    params = json.load(open(os.path.join(nizkp, "params.json")))
    assert params["group"] == {"kind": "ec", "curve": "P-256"} and params["vbitlenro"] == 256
    assert os.path.getsize(os.path.join(nizkp, "Ciphertexts.bt")) == 5 + 2 * (5 + 40 * (15 + 2 * 33))
