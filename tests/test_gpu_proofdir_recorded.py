"""GPU suite: whole proof directories against their recorded bytes (tests/golden/proofdir_sessions.json, written by
tools/record_proofdir_sessions.py before proofdir.py was folded onto one byte-tree reader and one seed derivation).  Every case
-- K = 3 parties, threshold 2, N = 12, N_0 = 16; the 512-bit golden group and P-256; (kappa, omega) in {(1,1), (1,2), (2,1), (2,2)};
mixing plain and committed, shuffling committed, decryption alone; a failing party 2, plain and committed, and a wrong reply of
party 2 in the decryption -- is written again from the same tapes: the SHA-256 of every file, the SHA-256 of verify_session's
vectors and its verdicts are the recorded ones.  The writers draw all their randomness from the tapes and the arithmetic is exact,
so the recording does not depend on the run (two recordings of the same commit were identical).

Wall time on an MI355X (one run): every case below 0.12 s in pytest's call durations; by the recorder's own clock 0.01 - 0.06 s
over the 512-bit group and 0.02 - 0.09 s over P-256 (the largest: mixing committed at kappa = omega = 2); the module's setup
(context, the two groups) 0.5 s; all 36 tests together about 2 s."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _recorder():
    spec = importlib.util.spec_from_file_location("record_proofdir_sessions", os.path.join(ROOT, "tools", "record_proofdir_sessions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _recorder()
with open(os.path.join(ROOT, "tests", "golden", "proofdir_sessions.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def mods(entry):
    import mirror
    return mirror.load(entry, ("proofdir", "randomsource"))


@pytest.fixture(scope="module")
def groups(vmn, gpu_ctx):
    return R.groups(vmn, gpu_ctx)


def test_the_fixture_holds_exactly_the_recorders_cases():
    assert sorted(RECORDED) == sorted(case[0] for case in R.cases()) and len(RECORDED) == 35


@pytest.mark.parametrize("case", R.cases(), ids=[case[0] for case in R.cases()])
def test_the_session_is_written_and_verified_as_recorded(case, mods, groups, tmp_path):
    want = RECORDED[case[0]]
    got = R.record(mods["proofdir"], mods["randomsource"], groups[case[1]], case, str(tmp_path / "nizkp"))
    assert sorted(got["files"]) == sorted(want["files"])
    assert [name for name in want["files"] if got["files"][name] != want["files"][name]] == []
    assert got["vectors"] == want["vectors"]
    verdicts = {key: got[key] for key in ("accepted", "verdicts", "replaced", "valid_proofs", "decryption", "correct")}
    assert verdicts == {key: want[key] for key in verdicts}
    name, _, _, _, session_type, _, active, failing, tampered = case
    parties = 0 if session_type == "decryption" else active
    assert got["accepted"] and got["verdicts"] == [l not in failing for l in range(1, parties + 1)] and got["replaced"] == list(failing)
    if session_type != "shuffling":
        assert got["decryption"] is True and got["correct"] == [True, True, not tampered, True]
