"""GPU suite: whole sessions under a public key of width kappa = 2 through proofdir.write_session / proofdir.verify_session with
keywidth: mixing, shuffling (plain and committed with N_0 = 40) and decryption, K = 3 parties, threshold 2, N = 30, omega in
{1, 3}, over the 512-bit golden group and over P-256.

What is compared with what: every file the key width changes with the trees tests/keyed_layout_ref.py builds from Python
integers (the list, the key, the polynomial, the factors and the plaintexts from values the integer restatement
tests/keyed_decrypt_ref.py computes; F', k_F, the decryption commitment and reply, whose values come from the provers' random
source, by decoding them and building them again); PoS.s / CCPoS.s, Dec.s, Dec.v and bas.y_l with hashlib over the same files;
the plaintexts with the restatement's opening of the last list under the kappa secrets.

Wall time on an MI355X (one run, pytest's call durations): the cases over the 512-bit group at most 0.33 s; over P-256 at most
0.9 s at omega = 1 and 2.5 s at omega = 3 where a decryption is restated (the restatement's curve arithmetic on Python integers,
not the GPU); the tool's test (two processes) 1.0 s; this module and tests/test_gpu_keyed_lists.py together 16.5 s."""
import json
import os

import pytest

from conftest import load_golden
from oracle.pyref_ec import Curve

import keyed_decrypt_ref as KD
import keyed_layout_ref as KL
import session_cases as S
import wide_decrypt_ref as WD
from session_cases import K, THR

pytestmark = pytest.mark.gpu

N, N0, KW = 30, 40, 2


@pytest.fixture(scope="module")
def mods(entry):
    import mirror
    return mirror.load(entry, ("proofdir", "randomsource", "fiatshamir", "native"))


@pytest.fixture(scope="module")
def groups(vmn, gpu_ctx):
    grpd, _ = load_golden(512)
    p, q, g = grpd["p"], grpd["q"], grpd["g"]
    M = vmn.ModPGroup(gpu_ctx, p, q, g)
    E = vmn.ECqPGroup(gpu_ctx, "P-256", java_widths=True)
    return {"modp": (M, S.gpu_params(M, "ModPGroup(512)", {"kind": "modp", "p": format(p, "x"), "q": format(q, "x"), "g": format(g, "x")}),
                     WD.adapter_modp(p, q), False),
            "p256": (E, S.gpu_params(E, "ECqPGroup(P-256)", {"kind": "ec", "curve": "P-256"}), WD.adapter_curve(Curve("P-256")), True)}


class Session:
    """A session of K parties, threshold THR, on a synthetic list of n ciphertexts of (G^kw)^w, written by write_session."""

    def __init__(self, pd, rs, group, nizkp, session_type, kw, w, active=THR, n0=0, failing=(), tag=b"keyed", n=N, keyed=True):
        G, params, self.K, self.curve = group
        self.G, self.nizkp, self.kw, self.w, self.n, self.vb, self.xb = G, nizkp, kw, w, n, G.nbytes, G.exp_bytes
        q, g = G.q, G.g
        tape = rs.InsecureShaRandomSource(tag + b"-tape", q)
        self.coeffs = [tape.ring_array(THR) for _ in range(kw)]
        share = lambda j, l: sum(c * pow(l, d, q) for d, c in enumerate(self.coeffs[j])) % q
        self.xs = [None] + [tuple(share(j, l) for j in range(kw)) for l in range(1, K + 1)]
        self.poly = [tuple(G.k_exp(g, self.coeffs[j][d]) for j in range(kw)) for d in range(THR)]
        self.y = self.poly[0]
        T = [G.ringArray(tape.ring_array(n)) for _ in range(kw * w)]
        M = [G.exp(g, G.ringArray(tape.ring_array(n))) for _ in range(kw * w)]
        self.W = [G.exp(g, t) for t in T] + [m.mul(G.exp(self.y[c % kw], t)) for c, (m, t) in enumerate(zip(M, T))]
        self.msgs = [m.toInts() for m in M]
        self.pkey = [g] * (kw * w) + list(self.y) * w
        more = {"keywidth": kw} if keyed else {}
        rows = (lambda x: x) if kw > 1 else (lambda x: x[0])                       # at key width 1 the interface takes the scalars
        self.params, plain = pd.write_session(nizkp, G, params, session_type, self.W, rows(self.y), rs.InsecureShaRandomSource(tag + b"-prover", q),
                                              K, THR, active=active, n0=n0, failing=failing, poly=[rows(c) for c in self.poly],
                                              shares=[None] + [rows(x) for x in self.xs[1:]], **more)
        self.plain = None if plain is None else [a.toInts() for a in plain]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def files_of(nizkp):
    return {name: read(os.path.join(nizkp, name)) for name in S.listing(nizkp)}


def item_span(buf, index):
    """(start, end) of child `index` of the node at the head of buf."""
    pos = 5
    for _ in range(index):
        _, pos = KL.decode(buf, pos)
    return pos, KL.decode(buf, pos)[1]


def hexk(pd, x):
    return "(" + ", ".join(pd._hex(e) for e in x) + ")"


# ---- round trips ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("session_type,n0", [("mixing", 0), ("mixing", N0), ("shuffling", 0), ("shuffling", N0), ("decryption", 0)])
@pytest.mark.parametrize("group", ["modp", "p256"])
def test_write_session_then_verify_session_accepts_and_every_file_is_the_restated_tree(group, session_type, n0, w, mods, groups, tmp_path):
    pd, rs, fs = mods["proofdir"], mods["randomsource"], mods["fiatshamir"]
    kw, Wc = KW, KW * w
    nizkp = str(tmp_path / "nizkp")
    I = Session(pd, rs, groups[group], nizkp, session_type, kw, w, n0=n0, tag=b"rt-%s-%d" % (session_type.encode(), n0))
    G, Kad, curve, vb, xb = I.G, I.K, I.curve, I.vb, I.xb
    tv = {}
    v = pd.verify_session(nizkp, G, I.params, vectors=tv)
    parties = 0 if session_type == "decryption" else THR
    assert v.accepted and v.verdicts == [True] * parties and v.valid_proofs == parties and v.replaced == frozenset()
    assert v.params == pd.SessionParams(session_type, "default", w, session_type != "shuffling", parties > 0, parties > 0)
    assert v.precomp == bool(n0) and tv["par.omega"] == str(w)
    assert json.load(open(os.path.join(nizkp, pd.PARAMS)))["keywidth"] == kw and I.params["width"] == w
    assert read(pd.width_file(nizkp)) == b"%d" % w
    # the same verdict with the key width given and params.json's ignored; a wrong one cannot read the key
    assert pd.verify_session(nizkp, G, dict(I.params, keywidth=1), keywidth=kw).accepted
    with pytest.raises(pd.SessionFormatError):
        pd.verify_session(nizkp, G, I.params, keywidth=1)
    # ---- the key and the input list
    assert read(pd.pk_file(nizkp)) == KL.public_key_tree(curve, vb, kw, G.g, I.y)
    assert tv["bas.pk"] == "(" + hexk(pd, [G.g] * kw) + ", " + hexk(pd, I.y) + ")"
    assert read(pd.l_file(nizkp, 0)) == KL.list_tree(curve, vb, kw, [a.toInts() for a in I.W])
    rho = pd.global_prefix(I.params)
    # ---- every party's proof: the nested items of its messages, and its seed with hashlib over the files
    g_tree, pk_tree = KL.element_tree(curve, vb, G.g), KL.ciphertext_tree(curve, vb, kw, I.pkey)
    H_bt = pd.derive_generators(G, I.params, rho, n0 or N).toByteTree() if parties else None
    out_of = lambda l: pd.l_file(nizkp, l) if os.path.exists(pd.l_file(nizkp, l)) else pd.ls_file(nizkp)
    for l in range(1, parties + 1):
        u_bt, L_in, L_out = read(pd.pc_file(nizkp, l)), read(out_of(l - 1) if l > 1 else pd.l_file(nizkp, 0)), read(out_of(l))
        if n0:
            keep = pd.read_keep_list(nizkp, l, n0, N)
            want = KL.shuffle_seed(rho, g_tree, pd._tree_prefix(G, H_bt, N), pd._tree_extract(G, u_bt, keep), pk_tree, L_in, L_out)
            assert tv["party"][l]["CCPoS.s"] == want.hex()
            com, rep, ci, ri = read(pd.ccposc_file(nizkp, l)), read(pd.ccposr_file(nizkp, l)), 1, 1      # (A', B'), (k_A, k_B, k_E)
        else:
            want = KL.shuffle_seed(rho, g_tree, H_bt, u_bt, pk_tree, L_in, L_out)
            assert tv["party"][l]["PoS.s"] == want.hex()
            com, rep, ci, ri = read(pd.posc_file(nizkp, l)), read(pd.posr_file(nizkp, l)), 5, 5          # .. F', .. k_F
        a, b = item_span(com, ci)
        halves = KL.decode(com, a)[0]
        flat = [KL.element_of(curve, e) for half in halves for e in KL.unnest(half, kw, w)]
        assert len(flat) == 2 * Wc and com[a:b] == KL.ciphertext_tree(curve, vb, kw, flat) and b == len(com)
        a, b = item_span(rep, ri)
        ring = [int.from_bytes(x, "big") for x in KL.unnest(KL.decode(rep, a)[0], kw, w)]
        assert len(ring) == Wc and rep[a:b] == KL.ring_tree(xb, kw, ring)
        # the single-link verifier on the same directory gives the same vectors
        if not os.path.exists(pd.l_file(nizkp, l)):
            os.link(pd.ls_file(nizkp), pd.l_file(nizkp, l))
        link = {}
        if n0:
            assert pd.verify_precomputed_shuffle(nizkp, l, G, I.params, I.pkey, n0, link, keywidth=kw)
        else:
            assert pd.verify_shuffle(nizkp, l, G, I.params, I.pkey, link, keywidth=kw)
        link.pop("der.rho")
        assert tv["party"][l] == link
    if session_type == "shuffling":
        assert v.decryption is None and I.plain is None and not os.path.exists(pd.plaintexts_file(nizkp))
        return
    # ---- the decryption: the restatement opens the last list under the kappa secrets
    last_bytes = read(pd.l_file(nizkp, parties))
    last = KL.read_list(curve, kw, w, last_bytes)
    u, vv = last[:Wc], last[Wc:]
    correct = [True] * (K + 1)
    assert v.decryption is True and v.correct == correct
    f_o = [None] + [KD.decryption_factors(Kad, kw, u, I.xs[l], K) for l in range(1, K + 1)]
    opened = KD.plaintexts(Kad, vv, KD.combine_decryption_factors(Kad, f_o, correct, K, THR))
    assert KL.read_wide_array(curve, kw, w, read(pd.plaintexts_file(nizkp))) == opened == I.plain
    assert read(pd.plaintexts_file(nizkp)) == KL.wide_array_tree(curve, vb, kw, opened)
    assert sorted(zip(*opened)) == sorted(zip(*I.msgs))
    if session_type == "decryption":
        assert opened == I.msgs
    poly_bt = read(pd.poly_file(nizkp))
    assert poly_bt == KL.polynomial_tree(curve, vb, kw, I.poly)
    factor_files = [read(pd.df_file(nizkp, l)) for l in range(1, K + 1)]
    assert factor_files == [KL.wide_array_tree(curve, vb, kw, f_o[l]) for l in range(1, K + 1)]
    ys = [None] + [tuple(Kad.exp(G.g, x) for x in I.xs[l]) for l in range(1, K + 1)]
    assert tv["bas.y_l"] == "(" + ",".join(hexk(pd, ys[l]) for l in range(1, THR + 1)) + ")"
    assert [tv["Dec.y_%d" % l] for l in range(1, K + 1)] == [hexk(pd, ys[l]) for l in range(1, K + 1)]
    seed = KL.decryption_seed(rho, curve, vb, kw, G.g, last_bytes, poly_bt, factor_files)
    assert tv["Dec.s"] == seed.hex()
    com_files = [read(pd.dfc_file(nizkp, l)) for l in range(1, K + 1)]
    assert tv["Dec.v"] == str(KL.decryption_challenge(rho, seed, com_files, int(I.params["vbitlenro"])))
    for l in range(1, K + 1):
        yp_t, Bp_t = KL.decode(com_files[l - 1])[0]
        yp = [KL.element_of(curve, e) for e in KL.unnest(yp_t, kw, 1)]
        Bp = [KL.element_of(curve, e) for e in KL.unnest(Bp_t, kw, w)]
        assert com_files[l - 1] == KL.commitment_tree(curve, vb, kw, yp, Bp)
        rep = read(pd.dfr_file(nizkp, l))
        kx = [int.from_bytes(x, "big") for x in KL.unnest(KL.decode(rep)[0], kw, 1)]
        assert len(kx) == kw and all(x < G.q for x in kx) and rep == KL.reply_tree(xb, kw, kx)


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["modp", "p256"])
def test_a_reply_row_wrong_under_one_key_fails_that_party_and_the_others_hold(group, mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    kw, w = KW, 3
    nizkp = str(tmp_path / "nizkp")
    I = Session(pd, rs, groups[group], nizkp, "decryption", kw, w, tag=b"reply")
    G = I.G
    assert pd.verify_session(nizkp, G, I.params).accepted

    def wrong_under_key_one(l, kx):
        return (kx[0], (kx[1] + 1) % G.q) if l == 2 else kx
    plain = pd.write_decryption(nizkp, G, I.params, I.pkey, I.W, I.poly, I.xs, rs.InsecureShaRandomSource(b"reply-again", G.q), K, THR,
                                keywidth=kw, tamper_reply=wrong_under_key_one)
    assert [a.toInts() for a in plain] == I.msgs
    v = pd.verify_session(nizkp, G, I.params)
    assert v.correct == [True, True, False, True] and v.decryption is True and v.accepted
    assert KL.read_wide_array(I.curve, kw, w, read(pd.plaintexts_file(nizkp))) == I.msgs
    # with party 2 claimed correct its reply goes into the combined proof, which then fails
    with open(pd.cr_file(nizkp), "wb") as f:
        f.write(pd._booleans_tree([True] * (K + 1)))
    v = pd.verify_session(nizkp, G, I.params)
    assert v.decryption is False and not v.accepted


@pytest.mark.parametrize("w", [1, 3])
def test_a_factor_file_with_the_two_key_rows_swapped_fails(w, mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    kw = KW
    nizkp = str(tmp_path / "nizkp")
    I = Session(pd, rs, groups["modp"], nizkp, "decryption", kw, w, tag=b"swap")
    assert pd.verify_session(nizkp, I.G, I.params).accepted
    path = pd.df_file(nizkp, 1)
    good = read(path)
    rows = KL.read_wide_array(I.curve, kw, w, good)
    rows[0], rows[1] = rows[1], rows[0]
    bad = KL.wide_array_tree(I.curve, I.vb, kw, rows)
    assert len(bad) == len(good) and bad != good
    with open(path, "wb") as f:
        f.write(bad)
    v = pd.verify_session(nizkp, I.G, I.params)
    assert v.decryption is False and not v.accepted
    with open(path, "wb") as f:
        f.write(good)
    assert pd.verify_session(nizkp, I.G, I.params).accepted


@pytest.mark.parametrize("group", ["modp", "p256"])
def test_a_public_key_whose_first_half_is_not_g_g_stops(group, mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    kw = KW
    nizkp = str(tmp_path / "nizkp")
    I = Session(pd, rs, groups[group], nizkp, "decryption", kw, 1, tag=b"pk")
    G = I.G
    other = I.K.exp(G.g, 2)
    for first in ([G.g, other], [other, G.g]):
        with open(pd.pk_file(nizkp), "wb") as f:
            f.write(KL.ciphertext_tree(I.curve, I.vb, kw, first + list(I.y)))
        with pytest.raises(pd.SessionFormatError, match="Basic public key is not the standard generator!"):
            pd.verify_session(nizkp, G, I.params)
    # a key of width 1 (node(g, y_0)) is no element of the group of keys of width 2
    with open(pd.pk_file(nizkp), "wb") as f:
        f.write(KL.ciphertext_tree(I.curve, I.vb, 1, [G.g, I.y[0]]))
    with pytest.raises(pd.SessionFormatError, match="Could not read full El Gamal public key"):
        pd.verify_session(nizkp, G, I.params)
    with open(pd.pk_file(nizkp), "wb") as f:
        f.write(KL.public_key_tree(I.curve, I.vb, kw, G.g, I.y))
    assert pd.verify_session(nizkp, G, I.params).accepted


@pytest.mark.parametrize("n0", [0, N0])
def test_a_failing_party_is_replaced_by_its_input_and_the_chain_goes_on(n0, mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    kw, w = KW, 3
    nizkp = str(tmp_path / "nizkp")
    I = Session(pd, rs, groups["modp"], nizkp, "mixing", kw, w, active=3, n0=n0, failing={2}, tag=b"failing")
    v = pd.verify_session(nizkp, I.G, I.params)
    assert v.verdicts == [True, False, True] and v.replaced == frozenset({2}) and v.valid_proofs == 2 and v.accepted
    assert read(pd.l_file(nizkp, 2)) == read(pd.l_file(nizkp, 1))
    assert v.decryption is True
    got = KL.read_wide_array(I.curve, kw, w, read(pd.plaintexts_file(nizkp)))
    assert got == I.plain and sorted(zip(*got)) == sorted(zip(*I.msgs))


# ---- key width 1 through the new parameter ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,session_type,n0,w", [("modp", "mixing", 0, 1), ("modp", "mixing", N0, 3), ("p256", "mixing", 0, 3),
                                                     ("p256", "shuffling", N0, 1), ("modp", "decryption", 0, 3)])
def test_key_width_one_through_the_parameter_writes_the_directory_written_without_it(group, session_type, n0, w, mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    a, b = str(tmp_path / "with"), str(tmp_path / "without")
    Ia = Session(pd, rs, groups[group], a, session_type, 1, w, n0=n0, tag=b"one")
    Ib = Session(pd, rs, groups[group], b, session_type, 1, w, n0=n0, tag=b"one", keyed=False)
    fa, fb = files_of(a), files_of(b)
    assert sorted(fa) == sorted(fb) and "keywidth" not in Ia.params and Ia.params == Ib.params
    assert [name for name in fa if fa[name] != fb[name]] == []
    assert Ia.plain == Ib.plain
    for I, nizkp in ((Ia, a), (Ib, b)):
        assert pd.verify_session(nizkp, I.G, I.params).accepted and pd.verify_session(nizkp, I.G, I.params, keywidth=1).accepted


# ---- the tool ----------------------------------------------------------------------------------------------------------------------------
def test_vmnv_vectors_tool_on_a_session_under_a_key_of_width_two(entry, tmp_path):
    """tools/vmnv_vectors.py --demo --keywidth 2 writes params.json's "keywidth"; -session reads it from there."""
    import subprocess
    import sys
    from conftest import ROOT
    nizkp = str(tmp_path / "demo_session")
    tool = [sys.executable, os.path.join(ROOT, "tools", "vmnv_vectors.py")]
    out = subprocess.run(tool + ["--demo", nizkp, "-session", "-mix", "--parties", "3", "--threshold", "2", "--width", "3", "--keywidth", "2",
                                 "--curve", "P-256", "-n", "12"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert json.load(open(os.path.join(nizkp, "params.json")))["keywidth"] == 2 and read(os.path.join(nizkp, "width")) == b"3"
    assert "verdict of the mixing session: accepted" in text and text.count("\nTEST VECTOR\nPoS.s - ") == 2 and "\nTEST VECTOR\nDec.s - " in text
    pk = text.split("\nTEST VECTOR\nbas.pk - ")[1].split("\n")[1]
    assert pk.startswith("(((") and pk.count("(") == 7                       # ((g, g), (y_0, y_1)), every element a point (x, y)
    # the directory alone, verified again: the key width comes from params.json
    again = subprocess.run(tool + [nizkp, "-session", "-mix"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert again.returncode == 0 and "verdict of the mixing session: accepted" in again.stdout.decode()
