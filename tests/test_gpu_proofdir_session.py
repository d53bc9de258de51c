"""GPU suite: whole sessions through proofdir.write_session / proofdir.verify_session (MixNetElGamalVerifyFiatShamirSession.verify
:1318-1670): K = 3 parties, threshold 2, N = 7 and N = 12, over the 512-bit group of tests/golden/modp512.json at width 1 and
over P-256 at width 3.

What is compared with what: the plaintexts with the messages the list was made from; every per-party vector with what the
single-link verifiers (verify_shuffle, verify_precomputed_shuffle: pinned by tests/test_gpu_proofdir*.py against hashlib and
the oracles) return for that link of the same directory; the seed of a party that follows a failed one with the random
oracle (fiatshamir.Challenger: hashlib) over the bytes of the files it must have been hashed over.

Wall time on an MI355X (one run, pytest's call durations): every case but the tool's at most 0.21 s, the tool's test (six
processes) 2.5 s, the module 4.4 s with its set-up."""
import os

import pytest

from conftest import load_golden

import session_cases as S
from session_cases import K, THR

pytestmark = pytest.mark.gpu

N0 = 16


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
    return {"modp": (M, S.gpu_params(M, "ModPGroup(512)", {"kind": "modp", "p": format(p, "x"), "q": format(q, "x"), "g": format(g, "x")}), 1),
            "p256": (E, S.gpu_params(E, "ECqPGroup(P-256)", {"kind": "ec", "curve": "P-256"}), 3)}


def plaintexts_of(pd, G, nizkp, width, n):
    arrays = pd._read_wide_array(G, pd.plaintexts_file(nizkp), width, n)
    assert arrays is not None
    return [a.toInts() for a in arrays]


def link_vectors(pd, G, I, nizkp, l, n0):
    """(verdict, vectors) of the single-link verifier for party l, without the values that belong to the session."""
    tv = {}
    if n0:
        ok = pd.verify_precomputed_shuffle(nizkp, l, G, I.params, I.pkey, n0, tv)
    else:
        ok = pd.verify_shuffle(nizkp, l, G, I.params, I.pkey, tv)
    tv.pop("der.rho")
    return ok, tv


# ---- round trips ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group, session_type, n0, n, active", [
    ("modp", "mixing", 0, 7, 2), ("modp", "mixing", N0, 12, 2), ("modp", "shuffling", 0, 12, 3), ("modp", "decryption", 0, 7, 2),
    ("p256", "mixing", 0, 12, 2), ("p256", "mixing", N0, 7, 3), ("p256", "shuffling", N0, 12, 2), ("p256", "decryption", 0, 7, 2)])
def test_write_session_then_verify_session_accepts(group, session_type, n0, n, active, mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    G, params, width = groups[group]
    nizkp = str(tmp_path / "nizkp")
    I = S.gpu_session(pd, rs, G, params, nizkp, session_type, n, width, active=active, n0=n0, tag=b"rt-" + session_type.encode())
    tv = {}
    v = pd.verify_session(nizkp, G, I.params, vectors=tv)
    parties = 0 if session_type == "decryption" else active
    assert v.accepted and v.verdicts == [True] * parties and v.valid_proofs == parties and v.replaced == frozenset()
    assert v.params == pd.SessionParams(session_type, "default", width, session_type != "shuffling", parties > 0, parties > 0)
    assert v.active_threshold == active and v.precomp == bool(n0)
    # ---- the session's own vectors
    assert (tv["par.k"], tv["par.lambda"], tv["par.lambda.active"], tv["par.omega"]) == (str(K), str(THR), str(active), str(width))
    assert (tv["par.n_e"], tv["par.n_r"], tv["par.n_v"], tv["par.version"], tv["par.sid"]) == ("256", "100", "256", "3.1.0", "SessionID")
    assert tv["der.rho"] == pd.global_prefix(I.params).hex() and tv["bas.pk"] == "(" + pd._hex(G.g) + ", " + pd._hex(I.y) + ")"
    assert tv.get("par.N_0") == (str(n0) if n0 and parties else None)
    # ---- the decryption: Plaintexts.bt holds the messages the writer started from
    if session_type == "shuffling":
        assert v.decryption is None and I.plain is None and not os.path.exists(pd.plaintexts_file(nizkp)) and "Dec.s" not in tv
        assert os.path.exists(pd.ls_file(nizkp)) and os.path.exists(pd.l_file(nizkp, active)) == (not n0)
    else:
        assert v.decryption is True and v.correct == [True] * (K + 1) and tv["Dec.s"] and int(tv["Dec.v"]) > 0
        got = plaintexts_of(pd, G, nizkp, width, n)
        assert got == I.plain
        assert sorted(zip(*got)) == sorted(zip(*I.msgs))                            # the same messages, in the shuffled order
        if session_type == "decryption":
            assert got == I.msgs
        assert [tv["Dec.y_%d" % l] for l in range(1, THR + 1)] == _split(tv["bas.y_l"], THR)      # the keys y_1 .. y_threshold
    # ---- every party's vectors: those of the single-link verifier on the same directory
    assert sorted(tv.get("party", {})) == list(range(1, parties + 1))
    for l in range(1, parties + 1):
        if not os.path.exists(pd.l_file(nizkp, l)):                                 # a shuffling session's last committed list
            os.link(pd.ls_file(nizkp), pd.l_file(nizkp, l))
        ok, want = link_vectors(pd, G, I, nizkp, l, n0)
        assert ok and tv["party"][l] == want and ("CCPoS.s" if n0 else "PoS.s") in want, l


def test_the_n_sized_vectors_of_a_session(mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    G, params, width = groups["modp"]
    n = 7
    nizkp = str(tmp_path / "nizkp")
    I = S.gpu_session(pd, rs, G, params, nizkp, "mixing", n, width, tag=b"arrays")
    tv = {}
    assert pd.verify_session(nizkp, G, I.params, vectors=tv, with_arrays=True).accepted
    H = pd.derive_generators(G, I.params, pd.global_prefix(I.params), n)
    assert tv["bas.h"] == pd._arr(H)
    as_text = lambda path: "(" + ", ".join(pd._arr(c) for c in pd.read_ciphertexts(G, path, width)) + ")"
    assert tv["bas.L_0"] == as_text(pd.l_file(nizkp, 0))
    for l in (1, 2):
        want = {}
        assert pd.verify_shuffle(nizkp, l, G, I.params, I.pkey, want, with_arrays=True)
        assert want.pop("bas.h") == tv["bas.h"] and want.pop("der.rho") == tv["der.rho"]
        got = dict(tv["party"][l])
        assert got.pop("bas.L_l") == as_text(pd.l_file(nizkp, l))
        assert got.pop("u") == pd._arr(pd.parse_commitment(G, open(pd.pc_file(nizkp, l), "rb").read(), n))
        assert got == want and "PoS.B" in want and "PoS.k_E" in want


def _split(text, count):
    """The `count` elements of "(a,b)" where an element may itself be "(x, y)"."""
    body, out, depth, cur = text[1:-1], [], 0, ""
    for ch in body:
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
            continue
        depth += ch == "("
        depth -= ch == ")"
        cur += ch
    out.append(cur)
    assert len(out) == count
    return out


# ---- replacement: party 2 of 3 publishes an invalid proof ------------------------------------------------------------------------------
def test_a_failed_party_is_replaced_by_its_input_with_and_without_hashing_ahead(mods, groups, tmp_path, monkeypatch):
    pd, rs, fs, nat = mods["proofdir"], mods["randomsource"], mods["fiatshamir"], mods["native"]
    G, params, width = groups["modp"]
    n = 7
    nizkp = str(tmp_path / "nizkp")
    I = S.gpu_session(pd, rs, G, params, nizkp, "mixing", n, width, active=3, failing={2}, tag=b"replace")

    def check():
        tv = {}
        v = pd.verify_session(nizkp, G, I.params, vectors=tv)
        assert v.verdicts == [True, False, True] and v.replaced == frozenset({2}) and v.valid_proofs == 2 and v.accepted
        assert [(p.pos, p.replaced) for p in v.parties] == [(True, False), (False, True), (True, False)]
        assert v.decryption is True and plaintexts_of(pd, G, nizkp, width, n) == I.plain
        assert sorted(zip(*I.plain)) == sorted(zip(*I.msgs))
        return v, tv
    monkeypatch.delenv("VMN_SESSION_HASH_AHEAD", raising=False)
    v, tv = check()
    assert open(pd.l_file(nizkp, 2), "rb").read() == open(pd.l_file(nizkp, 1), "rb").read()
    # party 3's seed: hashed over L_1 as its input
    rho = pd.global_prefix(I.params)
    H = pd.derive_generators(G, I.params, rho, n)
    files = [open(f, "rb").read() for f in (pd.pc_file(nizkp, 3), pd.l_file(nizkp, 1), pd.l_file(nizkp, 3))]
    inst = fs._hdr(0, 6) + G.element_tree(G.g) + H.toByteTree() + files[0] + fs.product_element_tree(G, I.pkey) + files[1] + files[2]
    assert tv["party"][3]["PoS.s"] == fs.Challenger(rho, "sha256").challenge(inst, 256).hex()
    # ---- the same with hashing ahead turned off: equal verdict, equal vectors
    monkeypatch.setenv("VMN_SESSION_HASH_AHEAD", "0")
    assert check() == (v, tv)
    monkeypatch.delenv("VMN_SESSION_HASH_AHEAD")
    # ---- what a cheater would publish as L_2: a re-encryption of L_1 under a fresh permutation
    L1 = pd.read_ciphertexts(G, pd.l_file(nizkp, 1), width)
    tape = rs.InsecureShaRandomSource(b"cheater", G.q)
    fake = nat.reencrypt_native(G, I.pkey, L1, [nat.random_ring_array_native(G, tape, n, 100)], tape.permutation(n))
    pd.write_ciphertexts(pd.l_file(nizkp, 2), fake)
    assert open(pd.l_file(nizkp, 2), "rb").read() != files[1]
    v2, tv2 = check()
    assert v2 == v and tv2["party"][3] == tv["party"][3] and tv2["party"][2]["PoS.s"] != tv["party"][2]["PoS.s"]
    monkeypatch.setenv("VMN_SESSION_HASH_AHEAD", "0")
    assert check() == (v2, tv2)


def test_too_few_valid_proofs_is_not_accepted_and_the_decryption_is_still_checked(mods, groups, tmp_path):
    pd, rs = mods["proofdir"], mods["randomsource"]
    G, params, width = groups["modp"]
    nizkp = str(tmp_path / "nizkp")
    I = S.gpu_session(pd, rs, G, params, nizkp, "mixing", 12, width, active=2, failing={1, 2}, tag=b"too-few")
    tv = {}
    v = pd.verify_session(nizkp, G, I.params, vectors=tv)
    assert v.verdicts == [False, False] and v.replaced == frozenset({1, 2}) and v.valid_proofs == 0 and not v.accepted
    assert v.decryption is True and v.correct == [True] * (K + 1) and tv["Dec.s"]
    assert plaintexts_of(pd, G, nizkp, width, 12) == I.msgs                         # nobody shuffled: L_0 was decrypted


def test_tampered_files_of_an_honest_session(mods, groups, tmp_path):
    pd, rs, fs = mods["proofdir"], mods["randomsource"], mods["fiatshamir"]
    G, params, width = groups["p256"]
    n = 7
    nizkp = str(tmp_path / "nizkp")
    I = S.gpu_session(pd, rs, G, params, nizkp, "mixing", n, width, tag=b"tamper")
    assert pd.verify_session(nizkp, G, I.params).accepted
    # ---- one flipped byte in Plaintexts.bt: every party valid, the session rejected
    path = pd.plaintexts_file(nizkp)
    good = open(path, "rb").read()
    bad = bytearray(good)
    bad[-1] ^= 1
    open(path, "wb").write(bytes(bad))
    v = pd.verify_session(nizkp, G, I.params)
    assert v.verdicts == [True, True] and v.valid_proofs == 2 and v.decryption is False and not v.accepted
    open(path, "wb").write(good)
    # ---- a truncated proofs/Ciphertexts01.bt: party 1 fails as its single link fails, party 2 is verified against L_0
    path = pd.l_file(nizkp, 1)
    good = open(path, "rb").read()
    open(path, "wb").write(good[:-3])
    assert not pd.verify_shuffle(nizkp, 1, G, I.params, I.pkey)
    tv = {}
    v = pd.verify_session(nizkp, G, I.params, vectors=tv)
    assert v.verdicts == [False, False] and v.replaced == frozenset({1, 2}) and not v.accepted
    assert "PoS.s" not in tv["party"][1]                                             # no list, no instance: nothing was hashed
    rho = pd.global_prefix(I.params)
    H = pd.derive_generators(G, I.params, rho, n)
    files = [open(f, "rb").read() for f in (pd.pc_file(nizkp, 2), pd.l_file(nizkp, 0), pd.l_file(nizkp, 2))]
    inst = fs._hdr(0, 6) + G.element_tree(G.g) + H.toByteTree() + files[0] + fs.product_element_tree(G, I.pkey) + files[1] + files[2]
    assert tv["party"][2]["PoS.s"] == fs.Challenger(rho, "sha256").challenge(inst, 256).hex()
    open(path, "wb").write(good)
    assert pd.verify_session(nizkp, G, I.params).accepted
    # ---- a session file gone: not a verdict
    os.remove(pd.type_file(nizkp))
    with pytest.raises(pd.SessionFormatError):
        pd.verify_session(nizkp, G, I.params)


# ---- the tool ----------------------------------------------------------------------------------------------------------------------------
def test_vmnv_vectors_tool_on_a_session(entry, tmp_path):
    import subprocess
    import sys
    from conftest import ROOT
    nizkp = str(tmp_path / "demo_session")
    tool = [sys.executable, os.path.join(ROOT, "tools", "vmnv_vectors.py")]
    out = subprocess.run(tool + ["--demo", nizkp, "-session", "-mix", "--parties", "3", "--threshold", "2", "--active", "3", "--width", "2",
                                 "--curve", "P-256", "-n", "12"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    for name in ("par.k", "par.lambda", "par.version", "par.omega", "bas.pk", "bas.y_l", "der.rho", "PoS.s", "PoS.v", "Dec.s", "Dec.v"):
        assert f"\nTEST VECTOR\n{name} - " in text, name
    assert text.count("\nTEST VECTOR\npar.lambda - ") == 2 and text.count("\nTEST VECTOR\nPoS.s - ") == 3
    order = [text.index(s) for s in ("par.k - ", "par.version - ", "bas.pk - ", "der.rho - ", "BEGIN PARTY 1 #", "END PARTY 1 #",
                                     "BEGIN PARTY 3 #", "END PARTY 3 #", "Dec.s - ", "party 1: valid", "party 3: valid",
                                     "verdict of the mixing session: accepted")]
    assert order == sorted(order)
    assert "bas.L_0" not in text and "bas.h" not in text                             # the N-sized ones only with --arrays
    # the options of the reference's tool: a type that is not the proof's, the decryption alone, a missing session file
    run = lambda *more: subprocess.run(tool + [nizkp, "-session"] + list(more), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = run("-shuffle")
    assert out.returncode == 2 and b"Attempting to verify proof of shuffling, but proof is a proof of mixing!" in out.stdout
    out = run("-mix", "-nopos", "-t", "Dec")
    assert out.returncode == 0 and b"BEGIN PARTY" not in out.stdout and b"Dec.s - " in out.stdout and b"PoS.s" not in out.stdout
    assert run("-mix", "-width", "3").returncode == 2
    out = run("-mix", "--arrays", "-t", "bas,u")
    assert out.returncode == 0 and all(b"\nTEST VECTOR\n" + name + b" - " in out.stdout for name in (b"bas.h", b"bas.L_0", b"bas.L_1", b"bas.L_3", b"u"))
    assert b"BEGIN PARTY" not in out.stdout and b"PoS.s" not in out.stdout
    os.remove(os.path.join(nizkp, "type"))
    out = run("-mix")
    assert out.returncode == 2 and b"Can not find type file" in out.stdout


# ---- the three verifiers and their cores on the links of a session --------------------------------------------------------------------
@pytest.mark.parametrize("group", ["modp", "p256"])
def test_the_cores_on_loaded_inputs_give_what_the_wrappers_give(group, mods, groups, tmp_path):
    pd, rs, fs = mods["proofdir"], mods["randomsource"], mods["fiatshamir"]
    G, params, width = groups[group]
    n = 12
    rho = pd.global_prefix(dict(params, auxsid="default"))
    chal = fs.Challenger(rho, "sha256")
    g_tree = G.element_tree(G.g)
    for n0 in (0, N0):
        nizkp = str(tmp_path / ("nizkp%d" % n0))
        I = S.gpu_session(pd, rs, G, params, nizkp, "mixing", n, width, n0=n0, tag=b"cores%d" % n0)
        pk_tree = fs.product_element_tree(G, I.pkey)
        H = pd.derive_generators(G, I.params, rho, n0 or n)
        lists = [pd.read_ciphertexts(G, pd.l_file(nizkp, l), width) for l in range(3)]
        data = [open(pd.l_file(nizkp, l), "rb").read() for l in range(3)]
        for l in (1, 2):
            ok, want = link_vectors(pd, G, I, nizkp, l, n0)
            assert ok
            u_bt = open(pd.pc_file(nizkp, l), "rb").read()
            U = pd.parse_commitment(G, u_bt, n0 or n)
            got = {}
            if n0:
                assert pd.posc_core(nizkp, l, G, I.params, H, U, n0, lambda: chal.challenge(fs._hdr(0, 3) + g_tree + H.toByteTree() + u_bt, 256), got)
                keep = pd.read_keep_list(nizkp, l, n0, n)
                U_s, H_s = U.extract(keep), H.copyOfRange(0, n)
                assert pd._tree_extract(G, u_bt, keep) == U_s.toByteTree() and pd._tree_prefix(G, H.toByteTree(), n) == H_s.toByteTree()
                inst = fs._hdr(0, 6) + g_tree + H_s.toByteTree() + U_s.toByteTree() + pk_tree + data[l - 1] + data[l]
                assert pd.ccpos_core(nizkp, l, G, I.params, I.pkey, H_s, U_s, lists[l - 1], lists[l], lambda: chal.challenge(inst, 256), got)
            else:
                inst = fs._hdr(0, 6) + g_tree + H.toByteTree() + u_bt + pk_tree + data[l - 1] + data[l]
                assert pd.pos_core(nizkp, l, G, I.params, I.pkey, lists[l - 1], lists[l], H, U, lambda: chal.challenge(inst, 256), got)
                assert got["verdicts(A,B,C,D,F)"] == str((True,) * 5)
            assert got == want
        tv, got = {}, {}
        assert pd.verify_decryption(nizkp, G, I.params, I.pkey, pd.l_file(nizkp, 2), tv)
        assert pd.dec_core(nizkp, G, I.params, I.pkey, lists[2], data[2], got) == (True, [True] * (K + 1)) and got == tv
        assert not pd.verify_decryption(nizkp, G, I.params, I.pkey, pd.l_file(nizkp, 1))
        assert not pd.verify_decryption(nizkp, G, I.params, I.pkey, os.path.join(nizkp, "absent.bt"))
