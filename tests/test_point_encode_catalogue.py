"""CPU suite: tests/point_encode_cases.py, the restatement of the message encoding over curve groups, checked against itself,
against libcrypto (every encoded point is on its curve: EC_POINT_is_on_curve) and against the pinned fixture
tests/golden/point_encode.json.  The counter coverage the GPU suite relies on -- accepted counters 0, 1, 2, 3 and one >= 6 in
every sample -- is asserted here for every curve used."""
import ctypes
import json
import os

import pytest

import encode_cases as ec
import named_curves as nc
import point_encode_cases as pe

GOLDEN = os.path.join(nc.ROOT, "tests", "golden", "point_encode.json")
CURVES = sorted({name.replace("-java", "") for name in pe.GPU_CURVES})


def test_the_encode_length_of_all_26_names_and_the_cofactor():
    for name in nc.NAMES:
        cv = nc.openssl_curve(name)
        b = cv["p"].bit_length()
        assert pe.encode_length(cv["p"]) == pe.ENCODE_LENGTH[b] == ec.encode_length(cv["p"]) - 1 >= 1, name
        assert cv["h"] == 1, name                                        # a point on the curve is a group element
        assert 1 << (8 * (pe.encode_length(cv["p"]) + 5)) <= 1 << (b - 2) < cv["p"]
    assert pe.encode_length(1 << 47) == 0 and pe.encode_length((1 << 50) - 27) == 1 and pe.encode_length(3) == 0


@pytest.mark.parametrize("name", CURVES)
def test_encoded_points_are_on_the_curve_have_the_smaller_root_and_decode(name):
    cv = pe.curve(name)
    p, L = cv["p"], pe.encode_length(cv["p"])
    lib = nc.libcrypto()
    grp = ctypes.c_void_p(lib.EC_GROUP_new_by_curve_name(lib.OBJ_sn2nid(nc.OPENSSL_SN[name].encode())))
    ctx, pt = ctypes.c_void_p(lib.BN_CTX_new()), ctypes.c_void_p(lib.EC_POINT_new(grp))
    nb = (p.bit_length() + 7) // 8
    for ncomp in pe.NCOMPS:
        for msg in pe.messages(name, ncomp):
            points = pe.encode_message(msg, name, ncomp)
            for piece, P in zip(ec.pieces(msg, ncomp, L), points):
                x, y = P
                c = pe.encode_piece(piece, name)[1]
                assert pe.on_curve(P, cv) and 0 < y <= p - y and pe.rhs(x, cv) != 0
                assert x == 256 * ec.value_of(piece, L) + c and 0 < x < 1 << (8 * (L + 5))
                assert all(pe.point_at(x - c + k, cv) is None for k in range(c)), "the counter is not the least"
                bx, by = (ctypes.c_void_p(lib.BN_bin2bn(v.to_bytes(nb, "big"), nb, None)) for v in (x, y))
                assert lib.EC_POINT_set_affine_coordinates(grp, pt, bx, by, ctx) == 1 and lib.EC_POINT_is_on_curve(grp, pt, ctx) == 1
                assert pe.decode_point(P, name) == (piece, True) == pe.decode_point(pe.negated(P, name), name)
            line, wf, utf8 = pe.decode_line(points, name)
            assert line == msg + b"\n" and wf and utf8 == ec.utf8_wellformed(msg)


@pytest.mark.parametrize("name", CURVES)
def test_every_sample_holds_the_counters_0_1_2_3_and_one_of_six_or_more(name):
    cm = pe.counter_messages(name)
    assert [pe.encode_piece(cm[k], name)[1] for k in (0, 1, 2, 3)] == [0, 1, 2, 3] and pe.encode_piece(cm[6], name)[1] >= 6
    for ncomp in pe.NCOMPS:
        pool = len(pe.messages(name, ncomp))
        counters = set(pe.sample_counters(name, ncomp, 63))              # (63 lines hold the whole pool)
        assert pool <= 63 and {0, 1, 2, 3} <= counters and max(counters) >= 6, (name, ncomp, sorted(counters))
        first = pe.sample_counters(name, ncomp, 3)                       # the unlucky lane between lucky ones, in the first wave
        assert first[0] == 0 and first[ncomp] >= 6


@pytest.mark.parametrize("name", CURVES)
def test_crafted_points(name):
    cv = pe.curve(name)
    L = pe.encode_length(cv["p"])
    for P in pe.ill_formed_points(name):
        assert pe.on_curve(P, cv) and pe.decode_point(P, name) == (b"", False) == pe.decode_point(pe.negated(P, name), name)
    P, c = pe.encode_piece(b"twice", name)
    Q = pe.other_counter(b"twice", name)
    assert Q[0] // 256 == P[0] // 256 and Q[0] % 256 > c and pe.on_curve(Q, cv) and pe.decode_point(Q, name) == (b"twice", True)
    for payload in ec.BAD_UTF8 + ec.STRIPPED + (ec.C3_0A_A9,):
        assert pe.decode_point(pe.encode_piece(payload, name)[0], name) == (payload, True)
    line, wf, utf8 = pe.decode_line([pe.encode_piece(ec.C3_0A_A9, name)[0]], name)
    assert (line, wf, utf8) == (b"\xc3\xa9\n", True, False)
    cols, first = pe.encode_text(b"ok\n" + b"x" * (2 * L + 1) + b"\n", name, 2)
    assert cols is None and first == 1


def test_the_utf8_restatement_against_bytes_decode():
    samples = list(ec.BAD_UTF8) + list(ec.STRIPPED) + [ec.C3_0A_A9, ec.EURO, ec.G_CLEF, ec.E_ACUTE, ec.G_CLEF[:3], b"", b"plain"]
    samples += [ec.stream(b"point-encode/utf8/%d" % i, 1 + i % 7) for i in range(300)]
    for data in samples:
        try:
            data.decode("utf-8")
            want = True
        except UnicodeDecodeError:
            want = False
        assert ec.utf8_wellformed(data) == want, data


def test_the_pinned_fixture():
    """tests/golden/point_encode.json guards the rule against drift: written once by point_encode_cases.golden_records()."""
    assert json.load(open(GOLDEN)) == pe.golden_records()
    for rec in pe.golden_records():
        P = (int(rec["x"], 16), int(rec["y"], 16))
        assert pe.decode_point(P, rec["curve"]) == (bytes.fromhex(rec["message"]), True)
