"""CPU suite: the control flow of a session's verification (verificatum-vmn_amd/proofdir.py: run_session, the session files,
write_session's file placement) over stub engines and hand-made files (tests/session_cases.py).  No GPU: the rules of
MixNetElGamalVerifyFiatShamirSession.verify (:1318-1670) -- which check stops the verification, which party is skipped, what a
failed party's successor is given, what is counted -- are properties of the loop, not of the proofs."""
import os

import pytest

import session_cases as S
from session_cases import K, THR


@pytest.fixture(scope="module")
def pd(entry):
    import mirror
    return mirror.load(entry, ("proofdir",))["proofdir"]


def run(pd, nizkp, script=None, expected=None, params=None, stats=None, vectors=None):
    stub = S.StubEngines(pd, script)
    verdict = pd.run_session(nizkp, S.TinyGroup(), params or S.tiny_params(), expected or pd.SessionParams(), stub.engines,
                             vectors, False, stats)
    return verdict, stub


def fails(pd, nizkp, message, **kw):
    stub = S.StubEngines(pd)
    with pytest.raises(pd.SessionFormatError) as err:
        pd.run_session(nizkp, S.TinyGroup(), kw.pop("params", None) or S.tiny_params(), kw.pop("expected", None) or pd.SessionParams(),
                       stub.engines)
    assert message in str(err.value)
    assert not [c for c in stub.names() if c in ("PoS", "PoSC", "CCPoS", "dec")], stub.calls
    return stub


@pytest.fixture
def nizkp(pd, tmp_path):
    path = str(tmp_path / "nizkp")
    S.tiny_session(pd, path)
    return path


# ---- the small files ---------------------------------------------------------------------------------------------------------------
def test_small_files_round_trip(pd, tmp_path):
    path = str(tmp_path / "f")
    pd.write_string(path, "mixing")
    assert open(path, "rb").read() == b"mixing" and pd.read_string(path) == "mixing"
    pd.write_int(path, 12)
    assert open(path, "rb").read() == b"12" and pd.read_string(path) == "12"
    open(path, "wb").write(b"  default_1\r\n")
    assert pd.read_string(path) == "default_1"
    pd.write_string(path, "grün")
    assert open(path, "rb").read() == "grün".encode("utf-8") and pd.read_string(path) == "grün"
    assert os.path.basename(pd.at_file("d")) == "activethreshold" and os.path.basename(pd.mc_file("d")) == "maxciph"
    assert pd.ls_file("d") == os.path.join("d", "ShuffledCiphertexts.bt")
    assert [os.path.basename(f("d")) for f in (pd.version_file, pd.type_file, pd.auxsid_file, pd.width_file)] == \
        ["version", "type", "auxsid", "width"]


# ---- every failStop: SessionFormatError, and no proof engine runs --------------------------------------------------------------------
def test_the_honest_stub_session_is_accepted(pd, nizkp):
    v, stub = run(pd, nizkp)
    assert v.accepted and v.verdicts == [True, True] and v.valid_proofs == 2 and v.decryption is True
    assert v.params == pd.SessionParams("mixing", "default", 1, True, True, True) and v.active_threshold == 2 and not v.precomp
    assert v.replaced == frozenset() and v.correct == [False, True, True, True]
    assert [c for c in stub.names() if c != "read_list"] == ["derive_generators", "PoS", "PoS", "dec"]


def test_a_missing_or_unknown_type_stops(pd, nizkp):
    os.remove(pd.type_file(nizkp))
    fails(pd, nizkp, "Can not find type file")
    pd.write_string(pd.type_file(nizkp), "mixnet")
    fails(pd, nizkp, "Unknown type of proof! (mixnet)")


def test_a_type_other_than_the_expected_one_stops(pd, nizkp):
    fails(pd, nizkp, "Attempting to verify proof of shuffling, but proof is a proof of mixing!", expected=pd.SessionParams(type="shuffling"))
    assert run(pd, nizkp, expected=pd.SessionParams(type="mixing"))[0].accepted


def test_a_wrong_version_stops(pd, nizkp):
    pd.write_string(pd.version_file(nizkp), "3.0.4")
    fails(pd, nizkp, "Expected package version 3.1.0 but the proof was created by a package with version 3.0.4!")
    os.remove(pd.version_file(nizkp))
    fails(pd, nizkp, "Can not find version file")


def test_a_bad_auxsid_stops(pd, nizkp):
    fails(pd, nizkp, "does not match the one in the proof", expected=pd.SessionParams(auxsid="other"))
    pd.write_string(pd.auxsid_file(nizkp), "not valid!")
    fails(pd, nizkp, "Invalid auxiliary session identifier")
    os.remove(pd.auxsid_file(nizkp))
    fails(pd, nizkp, "Can not find auxsid file")


def test_the_auxsid_of_the_proof_goes_into_the_prefix(pd, nizkp):
    pd.write_string(pd.auxsid_file(nizkp), "second_1")
    tv = {}
    v, _ = run(pd, nizkp, vectors=tv)
    assert v.params.auxsid == "second_1"
    assert tv["der.rho"] == pd.global_prefix(S.tiny_params(auxsid="second_1")).hex() != pd.global_prefix(S.tiny_params()).hex()


def test_width_mismatch_in_each_of_the_three_conventions(pd, nizkp):
    pd.write_int(pd.width_file(nizkp), 2)
    assert run(pd, nizkp, expected=pd.SessionParams(width=-1))[0].params.width == 2         # < 0: the proof's width
    fails(pd, nizkp, "does not match the width in the protocol info file", expected=pd.SessionParams(width=0))      # 0: the default
    assert run(pd, nizkp, expected=pd.SessionParams(width=0), params=S.tiny_params(width=2))[0].params.width == 2
    fails(pd, nizkp, "The given width does not match the width in the proof!", expected=pd.SessionParams(width=3))   # > 0: itself
    assert run(pd, nizkp, expected=pd.SessionParams(width=2))[0].params.width == 2
    pd.write_int(pd.width_file(nizkp), 0)
    fails(pd, nizkp, "Width is not positive!")
    pd.write_string(pd.width_file(nizkp), "two")
    fails(pd, nizkp, "Can not parse width given in file!")


def test_an_active_threshold_outside_its_range_stops(pd, nizkp):
    pd.write_int(pd.at_file(nizkp), K + 1)
    fails(pd, nizkp, "Active threshold is larger than the number of mix-servers!")
    pd.write_int(pd.at_file(nizkp), THR - 1)
    fails(pd, nizkp, "Active threshold is smaller than threshold!")
    os.remove(pd.at_file(nizkp))
    fails(pd, nizkp, "Can not find active threshold file")


def test_an_unparsable_maxciph_stops(pd, nizkp):
    pd.write_string(pd.mc_file(nizkp), "many")
    stub = fails(pd, nizkp, "Can not parse maxciph file!")
    assert "derive_generators" not in stub.names()
    pd.write_int(pd.mc_file(nizkp), S.StubEngines.N - 1)                           # fewer than there are ciphertexts
    stub = fails(pd, nizkp, "Too few generators have been derived!")
    assert "derive_generators" not in stub.names()


def test_a_basic_public_key_that_is_not_g_stops(pd, nizkp):
    open(pd.pk_file(nizkp), "wb").write(b"4,13")
    fails(pd, nizkp, "Basic public key is not the standard generator!")
    open(pd.pk_file(nizkp), "wb").write(b"garbage")
    fails(pd, nizkp, "Could not read full El Gamal public key")
    os.remove(pd.pk_file(nizkp))
    fails(pd, nizkp, "can not be found")


def test_a_polynomial_whose_element_0_is_not_the_key_stops(pd, nizkp):
    open(pd.poly_file(nizkp), "wb").write(b"3,5")
    fails(pd, nizkp, "Mismatching public keys!")
    assert run(pd, nizkp, expected=pd.SessionParams(dec=False))[0].accepted        # the polynomial is only read with a decryption
    os.remove(pd.poly_file(nizkp))
    fails(pd, nizkp, "Unable to read polynomial in exponent")


# ---- the party loop ------------------------------------------------------------------------------------------------------------------
def test_party_2_of_3_fails_and_party_3_is_given_its_input(pd, tmp_path):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, active=3)
    tv = {}
    v, stub = run(pd, nizkp, {("PoS", 2): False}, vectors=tv)
    assert v.verdicts == [True, False, True] and v.replaced == frozenset({2}) and v.valid_proofs == 2 and v.accepted
    assert [(p.l, p.pos, p.replaced) for p in v.parties] == [(1, True, False), (2, False, True), (3, True, False)]
    pos = {c[1]: c for c in stub.calls if c[0] == "PoS"}
    l1 = ("list", "Ciphertexts01.bt", b"L1")
    assert pos[2][3] == l1 and pos[2][4] == ("list", "Ciphertexts02.bt", b"L2")
    assert pos[3][3] is pos[2][3] and pos[3][4] == ("list", "Ciphertexts03.bt", b"L3")       # the input OBJECT, not a re-read
    assert sorted(c[1] for c in stub.calls if c[0] == "read_list") == ["Ciphertexts.bt", "Ciphertexts01.bt", "Ciphertexts02.bt", "Ciphertexts03.bt"]
    assert [c for c in stub.calls if c[0] == "dec"][0][1] == ("list", "Ciphertexts03.bt", b"L3")
    assert sorted(tv["party"]) == [1, 2, 3] and len({tv["party"][l]["PoS.s"] for l in (1, 2, 3)}) == 3


def test_the_last_list_is_taken_from_shuffledciphertexts_when_its_file_is_absent(pd, tmp_path):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, "shuffling")
    os.remove(pd.l_file(nizkp, 2))
    open(pd.ls_file(nizkp), "wb").write(b"LS")
    v, stub = run(pd, nizkp)
    assert v.accepted and v.decryption is None and v.params.dec is False
    assert [c for c in stub.calls if c[0] == "PoS"][1][4] == ("list", "ShuffledCiphertexts.bt", b"LS")
    # only for the LAST party: party 1's file absent fails party 1, whose output is replaced
    os.remove(pd.l_file(nizkp, 1))
    v, stub = run(pd, nizkp)
    assert v.verdicts == [False, True] and v.replaced == frozenset({1}) and not v.accepted
    assert [c[1] for c in stub.calls if c[0] == "PoS"] == [2]


def test_an_inactive_party_is_skipped_and_neither_counted_nor_replaced(pd, tmp_path):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, active=3)
    for f in (pd.pc_file, pd.posc_file, pd.posr_file):
        os.remove(f(nizkp, 2))
    tv = {}
    v, stub = run(pd, nizkp, vectors=tv)
    assert [p.l for p in v.parties] == [1, 3] and v.valid_proofs == 2 and v.replaced == frozenset() and v.accepted
    pos = [c for c in stub.calls if c[0] == "PoS"]
    assert [c[1] for c in pos] == [1, 3] and pos[1][3] is pos[0][4]                 # party 3 continues from party 1's output
    assert sorted(tv["party"]) == [1, 3]


def test_a_failed_posc_sets_the_commitment_to_the_generators_and_costs_the_verdict(pd, tmp_path):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, n0=5)
    tv = {}
    v, stub = run(pd, nizkp, {("PoSC", 1): False}, vectors=tv)
    assert v.precomp and v.verdicts == [False, True] and v.replaced == frozenset({1}) and not v.accepted
    assert (v.parties[0].posc, v.parties[0].ccpos) == (False, True) and (v.parties[1].posc, v.parties[1].ccpos) == (True, True)
    cc = {c[1]: c for c in stub.calls if c[0] == "CCPoS"}
    assert cc[1][2] == ("shrunk", ("range", ("H", 5), 5), 3)                        # the generators, all N_0 of them, shrunk
    assert cc[2][2][0] == "shrunk" and cc[2][2][1][0] == "U"                        # party 2: its own commitment
    assert cc[2][3] is cc[1][3]                                                     # and party 1's input
    assert ("derive_generators", 5) in stub.calls and stub.names().count("derive_generators") == 1
    # the seed of party 1's CCPoS was hashed over the generators' tree in the commitment's place
    import hashlib
    used = {l: next(p for k, j, p in stub.hashed if (k, j) == ("CCPoS", l) and hashlib.sha256(b"".join(p)).hexdigest() == tv["party"][l]["CCPoS.s"])
            for l in (1, 2)}
    h_bt = stub.derive_generators(None, None, 5)[1]
    assert used[1][2] == b"\x00\x00\x00\x00\x03" + h_bt[5:5 + 18] == used[1][1]
    assert used[2][2] == b"\x00\x00\x00\x00\x03" + b"\x01\x00\x00\x00\x01\x07" * 3 and used[2][4:] == [b"L0", b"L2"]


def test_too_few_valid_proofs_still_runs_the_decryption_and_is_not_accepted(pd, nizkp):
    v, stub = run(pd, nizkp, {("PoS", 1): False})
    assert v.valid_proofs == 1 < THR and "dec" in stub.names() and v.decryption is True and not v.accepted
    assert [c for c in stub.calls if c[0] == "dec"][0][1] == ("list", "Ciphertexts02.bt", b"L2")
    v, _ = run(pd, nizkp, {"dec": False})
    assert v.valid_proofs == 2 and v.decryption is False and not v.accepted


# ---- determineSessionParams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("session_type, cleared", [("mixing", ()), ("shuffling", ("dec",)), ("decryption", ("posc", "ccpos"))])
@pytest.mark.parametrize("flags", [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_the_table_of_determinesessionparams(pd, tmp_path, session_type, cleared, flags):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, session_type)
    dec, posc, ccpos = flags
    sp = pd.determine_session_params(nizkp, S.tiny_params(), pd.SessionParams(None, None, -1, dec, posc, ccpos), {})
    want = {"dec": dec and "dec" not in cleared, "posc": posc and "posc" not in cleared, "ccpos": ccpos and "ccpos" not in cleared}
    assert (sp.type, sp.auxsid) == (session_type, "default") and (sp.dec, sp.posc, sp.ccpos) == (want["dec"], want["posc"], want["ccpos"])
    assert sp.width == (1 if want["ccpos"] or want["dec"] else -1)                  # the width file is only read for ciphertexts


def test_the_decryption_alone_of_a_mixing_directory_starts_from_the_last_list(pd, tmp_path):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, active=3)
    v, stub = run(pd, nizkp, expected=pd.SessionParams(posc=False, ccpos=False))
    assert v.accepted and v.parties == [] and v.valid_proofs == 0 and v.decryption is True
    assert stub.calls == [("read_list", "Ciphertexts03.bt"), ("dec", ("list", "Ciphertexts03.bt", b"L3"), b"L3")]
    nizkp = str(tmp_path / "d")
    S.tiny_session(pd, nizkp, "decryption")
    v, stub = run(pd, nizkp)
    assert v.accepted and stub.calls == [("read_list", "Ciphertexts.bt"), ("dec", ("list", "Ciphertexts.bt", b"L0"), b"L0")]


# ---- hashing ahead -----------------------------------------------------------------------------------------------------------------------
def test_a_speculative_seed_is_discarded_when_the_party_before_fails(pd, tmp_path, monkeypatch):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, active=3)
    monkeypatch.delenv("VMN_SESSION_HASH_AHEAD", raising=False)
    stats, tv = {}, {}
    v, stub = run(pd, nizkp, {("PoS", 2): False}, stats=stats, vectors=tv)
    assert stats["ahead"] == [("shuffle", 1), ("shuffle", 2), ("shuffle", 3)]
    assert stats["used"] == [("shuffle", 1), ("shuffle", 2)] and stats["discarded"] == [("shuffle", 3)]
    of_3 = [parts for kind, l, parts in stub.hashed if (kind, l) == ("PoS", 3)]
    tails = [p[4:] for p in of_3]                # the one that was used, and the speculative one unless it was cancelled in time
    assert [b"L1", b"L3"] in tails and all(t in ([b"L1", b"L3"], [b"L2", b"L3"]) for t in tails) and len(tails) <= 2
    import hashlib
    assert tv["party"][3]["PoS.s"] == hashlib.sha256(b"".join(next(p for p in of_3 if p[4] == b"L1"))).hexdigest()
    # ---- off: nothing ahead, the same seeds
    monkeypatch.setenv("VMN_SESSION_HASH_AHEAD", "0")
    stats0, tv0 = {}, {}
    v0, stub0 = run(pd, nizkp, {("PoS", 2): False}, stats=stats0, vectors=tv0)
    assert stats0 == {"ahead": [], "used": [], "discarded": []} and v0 == v and tv0 == tv
    assert [(kind, l, p[4:]) for kind, l, p in stub0.hashed] == [("PoS", 1, [b"L0", b"L1"]), ("PoS", 2, [b"L1", b"L2"]), ("PoS", 3, [b"L1", b"L3"])]


def test_honest_parties_use_every_seed_that_was_hashed_ahead(pd, tmp_path, monkeypatch):
    nizkp = str(tmp_path / "n")
    S.tiny_session(pd, nizkp, n0=5)
    monkeypatch.delenv("VMN_SESSION_HASH_AHEAD", raising=False)
    stats = {}
    v, stub = run(pd, nizkp, stats=stats)
    assert v.accepted and sorted(stats["ahead"]) == sorted(stats["used"]) == [("PoSC", 1), ("PoSC", 2), ("shuffle", 1), ("shuffle", 2)]
    assert stats["discarded"] == [] and len(stub.hashed) == 4


# ---- write_session: which files, per type and flow ----------------------------------------------------------------------------------------
SMALL = ["FullPublicKey.bt", "auxsid", "proofs/activethreshold", "type", "version", "width"]


def proof_files(names, parties):
    return ["proofs/%s%02d.bt" % (n, l) for n in names for l in parties]


POS = ("PermutationCommitment", "PoSCommitment", "PoSReply")
CC = ("PermutationCommitment", "PoSCCommitment", "PoSCReply", "KeepList", "CCPoSCommitment", "CCPoSReply")
DEC = ["Plaintexts.bt", "proofs/PolynomialInExponent.bt"]


@pytest.mark.parametrize("session_type, n0, active, want", [
    ("shuffling", 0, 2, ["Ciphertexts.bt", "ShuffledCiphertexts.bt"] + proof_files(("Ciphertexts",) + POS, (1, 2))),
    ("shuffling", 5, 2, ["Ciphertexts.bt", "ShuffledCiphertexts.bt", "proofs/maxciph", "proofs/Ciphertexts01.bt"] + proof_files(CC, (1, 2))),
    ("shuffling", 5, 3, ["Ciphertexts.bt", "ShuffledCiphertexts.bt", "proofs/maxciph"] + proof_files(("Ciphertexts",), (1, 2)) + proof_files(CC, (1, 2, 3))),
    ("mixing", 0, 2, ["Ciphertexts.bt"] + DEC + proof_files(("Ciphertexts",) + POS, (1, 2))),
    ("mixing", 0, 3, ["Ciphertexts.bt"] + DEC + proof_files(("Ciphertexts",) + POS, (1, 2, 3))),
    ("mixing", 5, 2, ["Ciphertexts.bt", "proofs/maxciph"] + DEC + proof_files(("Ciphertexts",), (1, 2)) + proof_files(CC, (1, 2))),
    ("decryption", 0, 2, ["Ciphertexts.bt"] + DEC),
])
def test_write_session_places_the_files_of_each_type_and_flow(pd, tmp_path, session_type, n0, active, want):
    nizkp = str(tmp_path / "n")
    log = []
    params = S.tiny_session(pd, nizkp, session_type, active=active, n0=n0, log=log)
    assert S.listing(nizkp) == sorted(SMALL + want)
    assert pd.read_string(pd.type_file(nizkp)) == session_type and pd.read_string(pd.at_file(nizkp)) == str(active)
    assert pd.read_string(pd.width_file(nizkp)) == "1" and pd.read_string(pd.version_file(nizkp)) == "3.1.0"
    assert open(pd.pk_file(nizkp), "rb").read() == b"2,13"                          # (g, y): the key at width 1
    assert (params["k"], params["threshold"], params["N_0"], params["width"]) == (K, THR, n0, 1)
    if n0:
        assert pd.read_string(pd.mc_file(nizkp)) == "5"
    if session_type == "shuffling":
        assert open(pd.ls_file(nizkp), "rb").read() == b"L%d" % active
    if session_type == "mixing":
        assert open(pd.l_file(nizkp, active), "rb").read() == b"L%d" % active and log[-1] == ("decryption", "L%d" % active)
    if session_type == "decryption":
        assert log == [("inputs", [2, 13]), ("decryption", ["u", "v"])]
    # every written directory verifies under the stub engines
    v, _ = run(pd, nizkp)
    assert v.accepted and v.params.type == session_type and len(v.parties) == (0 if session_type == "decryption" else active)


@pytest.mark.parametrize("n0", [0, 5])
def test_write_session_with_a_failing_party_goes_on_from_its_input(pd, tmp_path, n0):
    nizkp = str(tmp_path / "n")
    log = []
    S.tiny_session(pd, nizkp, active=3, n0=n0, failing={2}, log=log)
    shuffles = [e for e in log if e[0] in ("shuffle", "committed")]
    assert [(e[1], e[2]) for e in shuffles] == [(1, ["u", "v"]), (2, "L1"), (2, "L1"), (3, "L1")]      # party 2 twice: the unrelated run
    assert open(pd.l_file(nizkp, 2), "rb").read() == b"L1"                          # what the honest parties keep as its output
    assert log[-1] == ("decryption", "L3")
    assert [n for n in S.listing(nizkp) if n.startswith("tmp")] == []
