"""The message encoding over curve groups and the text interface behind a curve session, restated on Python integers
(csrc/ec_encode_layout.h, csrc/ec_encode_kernels.h; csrc/vmnhip.hip: vmn_ec_group_encode_length / vmn_ec_arrays_from_textlines /
vmn_ec_arrays_to_textlines).  Never calls the library.  Shared by tests/test_point_encode_catalogue.py (the restatement checks
itself; no GPU), tests/test_point_encode_layout_host.py (the header as host code against it) and tests/test_gpu_point_texts.py
(the kernels against it, by exact equality).

The rule: b = bits(p), L = (b - 2) // 8 - 5; T = be32(|m|) || m || zeros on L + 4 bytes (|m| = 0: T[4] = 1); x = 256 int(T) + c
for the least c in 0..255 with x^3 + a x + b a nonzero square mod p; y = the smaller root.  decode: ill-formed (empty message) for
the point at infinity (None), for x >= 2^(8 (L + 5)) and for a length word of x // 256 above L; the counter and y are ignored.
Components, the removal of 0x0A / 0x0D and the UTF-8 verdict are those of tests/encode_cases.py."""
import functools

import encode_cases as ec
import named_curves as nc

# the curves of the GPU suite (-java: the reference's wider coordinates) and what each is there for
GPU_CURVES = ("P-192", "P-224", "secp224k1", "prime239v1", "P-256", "P-256-java", "brainpoolp256r1", "secp256k1", "P-384",
              "brainpoolp512r1", "P-521")
ENCODE_LENGTH = {192: 18, 224: 22, 239: 24, 256: 26, 320: 34, 384: 42, 512: 58, 521: 59}
NS = ec.NS
NCOMPS = ec.NCOMPS
COUNTER_CLASSES = (0, 1, 2, 3, 6)          # accepted counters every sample holds: 0, 1, 2, 3 and one that is >= 6


@functools.lru_cache(maxsize=None)
def curve(name: str) -> dict:
    """p, a, b (and the rest) of a reference name, from libcrypto."""
    return nc.openssl_curve(name.replace("-java", ""))


def encode_length(p: int) -> int:
    return max(0, (p.bit_length() - 2) // 8 - 5)


def sqrt_mod(a: int, p: int):
    """A square root of a mod the odd prime p, or None (a = 0: 0).  Tonelli-Shanks when p = 1 mod 4."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, x = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, tt = 0, t
        while tt != 1:
            tt, i = tt * tt % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, x = i, b * b % p, t * b * b % p, x * b % p
    return x


def rhs(x: int, cv: dict) -> int:
    return (x * x * x + cv["a"] * x + cv["b"]) % cv["p"]


def on_curve(P, cv: dict) -> bool:
    return P is None or (0 <= P[0] < cv["p"] and 0 <= P[1] < cv["p"] and (P[1] * P[1] - rhs(P[0], cv)) % cv["p"] == 0)


def point_at(x: int, cv: dict):
    """(x, the smaller root) when x^3 + a x + b is a nonzero square, else None."""
    r = rhs(x, cv)
    if r == 0:
        return None
    y = sqrt_mod(r, cv["p"])
    return None if y is None else (x, min(y, cv["p"] - y))


@functools.lru_cache(maxsize=None)
def encode_piece(piece: bytes, name: str):
    """(point, counter) of one piece of at most L bytes."""
    cv = curve(name)
    T = ec.value_of(piece, encode_length(cv["p"]))
    for c in range(256):
        P = point_at(256 * T + c, cv)
        if P is not None:
            return P, c
    raise AssertionError("no counter fits (chance 2^-256)")


def encode_message(msg: bytes, name: str, ncomp: int = 1):
    L = encode_length(curve(name)["p"])
    return [encode_piece(piece, name)[0] for piece in ec.pieces(msg, ncomp, L)]


def encode_text(text: bytes, name: str, ncomp: int):
    """(columns | None, first long line): ncomp columns of points."""
    L = encode_length(curve(name)["p"])
    lines = ec.split_lines(text)
    for i, line in enumerate(lines):
        if len(line) > ncomp * L:
            return None, i
    rows = [encode_message(line, name, ncomp) for line in lines]
    return [[row[c] for row in rows] for c in range(ncomp)], 0


def decode_point(P, name: str):
    """(message, well-formed)"""
    L = encode_length(curve(name)["p"])
    if P is None or P[0] >= 1 << (8 * (L + 5)):
        return b"", False
    T = (P[0] // 256).to_bytes(L + 4, "big")
    n = int.from_bytes(T[:4], "big")
    if n > L:
        return b"", False
    return T[4:4 + n], True


def decode_line(points, name: str):
    parts = [decode_point(P, name) for P in points]
    whole = b"".join(m for m, _ in parts)
    return whole.replace(b"\n", b"").replace(b"\r", b"") + b"\n", all(ok for _, ok in parts), ec.utf8_wellformed(whole)


def decode_text(columns, name: str):
    """(text, all_wellformed, all_utf8) of ncomp columns of n points each."""
    lines = [decode_line(row, name) for row in zip(*columns)]
    return b"".join(t for t, _, _ in lines), all(w for _, w, _ in lines), all(u for _, _, u in lines)


def point_bytes(P, vb: int) -> bytes:
    """x || y on vb bytes each; the point at infinity all 0xff (the arrays' export)."""
    return b"\xff" * (2 * vb) if P is None else P[0].to_bytes(vb, "big") + P[1].to_bytes(vb, "big")


def block(column, vb: int) -> bytes:
    return b"".join(point_bytes(P, vb) for P in column)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counter_messages(name: str):
    """{class: message} for the classes of COUNTER_CLASSES (6: the first message whose counter is >= 6), found by walking a
    hashed stream of line-safe messages of 1..L bytes.  A lane that needs seven rounds or more beside lanes that need one is
    where the search kernel can go wrong."""
    L = encode_length(curve(name)["p"])
    found = {}
    for i in range(100000):
        m = ec.line_safe(ec.stream(b"point-encode/counter/%s/%d" % (name.encode(), i), 1 + i % L))
        c = encode_piece(m, name)[1]
        k = 6 if c >= 6 else c
        if k in COUNTER_CLASSES and k not in found:
            found[k] = m
            if len(found) == len(COUNTER_CLASSES):
                return found
    raise AssertionError("the stream holds no message of every counter class")


def messages(name: str, ncomp: int):
    """encode_cases.messages(L, ncomp) and the counter messages, the unlucky one between two lucky ones."""
    L = encode_length(curve(name)["p"])
    cm = counter_messages(name)
    return [cm[0], cm[6], cm[1]] + ec.messages(L, ncomp) + [cm[2], cm[3]]


def sample_text(name: str, ncomp: int, n: int) -> bytes:
    """n lines drawn round-robin from messages(), ended by \\n."""
    pool = messages(name, ncomp)
    return b"".join(pool[i % len(pool)] + b"\n" for i in range(n))


def sample_counters(name: str, ncomp: int, n: int):
    """The counters the points of sample_text(name, ncomp, n) were accepted at."""
    L = encode_length(curve(name)["p"])
    return [encode_piece(piece, name)[1] for line in ec.split_lines(sample_text(name, ncomp, n)) for piece in ec.pieces(line, ncomp, L)]


def craft(name: str, length_word: int, tag: bytes):
    """A point of the curve whose x holds the given length word over a hashed tail: the free tail bytes are walked until an x is on
    the curve.  (Decoder inputs that no text produces.)"""
    cv = curve(name)
    L = encode_length(cv["p"])
    for k in range(1000):
        T = int.from_bytes(length_word.to_bytes(4, "big") + ec.stream(tag + b"/%d" % k, L), "big")
        P = point_at(256 * T + k % 256, cv)
        if P is not None:
            return P
    raise AssertionError("no x on the curve")


def ill_formed_points(name: str):
    """Points that hold no message: length words L + 1, 2^31 and 0xffffffff, an x >= 2^(8 (L + 5)), the point at infinity."""
    cv = curve(name)
    L = encode_length(cv["p"])
    out = [craft(name, n, b"point-encode/ill-formed") for n in (L + 1, 1 << 31, 0xffffffff)]
    x = (1 << (8 * (L + 5))) + 5
    while point_at(x, cv) is None:
        x += 1
    assert x < cv["p"]
    return out + [point_at(x, cv), None]


def negated(P, name: str):
    return None if P is None else (P[0], curve(name)["p"] - P[1])


def other_counter(piece: bytes, name: str):
    """A point with the T of encode_piece(piece) and a larger counter."""
    cv = curve(name)
    P, c = encode_piece(piece, name)
    for c2 in range(c + 1, 256):
        Q = point_at(P[0] - c + c2, cv)
        if Q is not None:
            return Q
    raise AssertionError("no second counter")


# the pinned fixture (tests/golden/point_encode.json): a few (curve, message) -> point, written by this restatement
GOLDEN_CASES = (("P-256", b""), ("P-256", b"vote"), ("P-256", "grüße €".encode()), ("P-224", b"vote"), ("secp256k1", b"vote"),
                ("brainpoolp256r1", b"\xff" * 26), ("P-521", b"A" * 59), ("prime239v1", b"\x00"))


def golden_records():
    out = []
    for name, msg in GOLDEN_CASES:
        P, c = encode_piece(msg, name)
        out.append({"curve": name, "message": msg.hex(), "x": format(P[0], "x"), "y": format(P[1], "x"), "counter": c})
    return out
