"""Helpers of the tests of the named curves (test_named_curves.py, test_gpu_named_curves.py): the reference's 26 curve names,
the curve table compiled into the library (csrc/vmnhip.hip kCurves) as the source spells it, libcrypto's constants for a name,
and the oracle's affine curve (oracle/pyref_ec.Curve) over a general a, built from the product's constants."""
import ctypes
import ctypes.util
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 26 names of the reference (demo/mixnet/.conf:151-176) -> OpenSSL's short name of the same curve (OBJ_sn2nid)
OPENSSL_SN = {
    "P-192": "prime192v1", "P-224": "secp224r1", "P-256": "prime256v1", "P-384": "secp384r1", "P-521": "secp521r1",
    **{"brainpoolp%dr1" % b: "brainpoolP%dr1" % b for b in (192, 224, 256, 320, 384, 512)},
    **{"prime192v%d" % v: "prime192v%d" % v for v in (1, 2, 3)},
    **{"prime239v%d" % v: "prime239v%d" % v for v in (1, 2, 3)},
    "prime256v1": "prime256v1",
    "secp192k1": "secp192k1", "secp192r1": "prime192v1", "secp224k1": "secp224k1", "secp224r1": "secp224r1",
    "secp256k1": "secp256k1", "secp256r1": "prime256v1", "secp384r1": "secp384r1", "secp521r1": "secp521r1",
}
NAMES = sorted(OPENSSL_SN)


def libcrypto():
    lib = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
    for f in ("EC_GROUP_new_by_curve_name", "EC_POINT_new", "BN_new", "BN_CTX_new", "BN_bin2bn", "EC_GROUP_get0_generator",
              "EC_GROUP_get0_order", "EC_GROUP_get0_cofactor"):
        getattr(lib, f).restype = ctypes.c_void_p
    lib.OBJ_sn2nid.argtypes = [ctypes.c_char_p]
    return lib


def _bn(lib, bn):
    buf = ctypes.create_string_buffer(80)
    n = lib.BN_bn2bin(ctypes.c_void_p(bn), buf)
    return int.from_bytes(buf.raw[:n], "big")


def openssl_curve(name):
    """p, a, b, gx, gy, n, h of a reference name, from libcrypto."""
    lib = libcrypto()
    nid = lib.OBJ_sn2nid(OPENSSL_SN[name].encode())
    assert nid > 0, name
    grp, ctx = ctypes.c_void_p(lib.EC_GROUP_new_by_curve_name(nid)), ctypes.c_void_p(lib.BN_CTX_new())
    p, a, b, x, y = (ctypes.c_void_p(lib.BN_new()) for _ in range(5))
    assert lib.EC_GROUP_get_curve(grp, p, a, b, ctx) == 1
    assert lib.EC_POINT_get_affine_coordinates(grp, ctypes.c_void_p(lib.EC_GROUP_get0_generator(grp)), x, y, ctx) == 1
    return dict(p=_bn(lib, p.value), a=_bn(lib, a.value), b=_bn(lib, b.value), gx=_bn(lib, x.value), gy=_bn(lib, y.value),
                n=_bn(lib, lib.EC_GROUP_get0_order(grp)), h=_bn(lib, lib.EC_GROUP_get0_cofactor(grp)))


def openssl_mul(name, k):
    """k G by libcrypto's EC_POINT_mul (None: the point at infinity)."""
    lib = libcrypto()
    grp = ctypes.c_void_p(lib.EC_GROUP_new_by_curve_name(lib.OBJ_sn2nid(OPENSSL_SN[name].encode())))
    pt, ctx = ctypes.c_void_p(lib.EC_POINT_new(grp)), ctypes.c_void_p(lib.BN_CTX_new())
    kb = k.to_bytes(80, "big")
    bn = ctypes.c_void_p(lib.BN_bin2bn(kb, len(kb), None))
    assert lib.EC_POINT_mul(grp, pt, bn, None, None, ctx) == 1
    if lib.EC_POINT_is_at_infinity(grp, pt):
        return None
    x, y = ctypes.c_void_p(lib.BN_new()), ctypes.c_void_p(lib.BN_new())
    assert lib.EC_POINT_get_affine_coordinates(grp, pt, x, y, ctx) == 1
    return _bn(lib, x.value), _bn(lib, y.value)


def library_table():
    """kCurves and kCurveAliases of csrc/vmnhip.hip as the source spells them: {name: dict(bits, S, NW, p, n, b, gx, gy, a)}
    (a = None where the entry does not name it: a = -3), {alias: name}."""
    src = open(os.path.join(ROOT, "verificatum-vmn_amd", "csrc", "vmnhip.hip")).read()
    body = src[src.index("static const CurveParams kCurves[] = {"):]
    body = body[:body.index("\n};")]
    table = {}
    for m in re.finditer(r'\{"([^"]+)",\s*(\d+),\s*(\d+),\s*(\d+),((?:\s*"[0-9a-f]+",?)+)\}', body):
        hexes = [int(h, 16) for h in re.findall(r'"([0-9a-f]+)"', m.group(5))]
        assert len(hexes) in (5, 6), m.group(1)
        table[m.group(1)] = dict(bits=int(m.group(2)), S=int(m.group(3)), NW=int(m.group(4)), p=hexes[0], n=hexes[1], b=hexes[2],
                                 gx=hexes[3], gy=hexes[4], a=hexes[5] if len(hexes) == 6 else None)
    al = src[src.index("kCurveAliases[][2] = {"):]
    al = al[:al.index("};")]
    aliases = dict(re.findall(r'\{"([^"]+)", "([^"]+)"\}', al))
    return table, aliases


def ecscalar():
    spec = importlib.util.spec_from_file_location("ecscalar_named", os.path.join(ROOT, "verificatum-vmn_amd", "ecscalar.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_curve(name):
    """oracle/pyref_ec.Curve over any named curve: the oracle's affine formulas already take a general a (self.a); its own
    table holds the four NIST curves only, so the constants come from the product's ecscalar.py (checked against libcrypto
    by test_named_curves.py)."""
    from oracle.pyref_ec import Curve
    es = ecscalar()
    c = es.curve(name)
    cur = Curve.__new__(Curve)
    cur.name, cur.p, cur.n, cur.b, cur.a = name, c["p"], c["n"], c["b"], es.curve_a(c)
    cur.g = (c["gx"], c["gy"])
    cur.nbytes = (cur.p.bit_length() + 7) // 8
    assert cur.on_curve(cur.g)
    return cur
