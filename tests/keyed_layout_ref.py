"""Test infrastructure: the files of a session under a public key of width kappa, restated on Python integers and `bytes`.

The rule (applied once more): under a key of width kappa the plaintext group is G^kappa
(MixNetElGamalVerifyFiatShamir.java:316-317), a ciphertext of width omega lives in ((G^kappa)^omega)^2, and an element, an array
or a ring element of a product is the node of its factors' trees.  So whatever has kappa * omega factors -- a half of a list, a
half of a ciphertext, the factors of a party, the plaintexts, B', k_F -- is

    [omega > 1: node(omega; ...)]  over  [kappa > 1: node(kappa; ...)]  over the factors' own trees,

factor c = l * kappa + j being the key j of plaintext component l.  kappa = 1 is the unkeyed form, omega = 1 the unkeyed form of
width kappa.  The generators and der.rho know nothing of kappa (:556-576, :158-189).

A group is described by (curve, vb): a modular group with leaves of vb bytes, or a curve with coordinates of vb bytes.  A group
element is an integer, or an affine point (x, y) / None for the point at infinity; a ring element an integer written on xb
bytes.  Nothing here imports the package: the random oracle is hashlib."""
import hashlib


def hdr(tag, n):
    return bytes([tag]) + int(n).to_bytes(4, "big")


def leaf(data):
    return hdr(1, len(data)) + bytes(data)


def node(children):
    return hdr(0, len(children)) + b"".join(children)


def nest(trees, kw):
    """The tree of kappa * omega factors given by their trees in flat order."""
    assert kw >= 1 and len(trees) % kw == 0
    omega = len(trees) // kw
    per_component = [trees[l * kw:(l + 1) * kw] for l in range(omega)]
    inner = [node(t) if kw > 1 else t[0] for t in per_component]
    return node(inner) if omega > 1 else inner[0]


# ---- sizes, from the rule alone ------------------------------------------------------------------------------------------------
def element_bytes(curve, vb):
    return 15 + 2 * vb if curve else 5 + vb


def line_bytes(curve, vb, kw, omega):
    """Bytes of one ciphertext: node(u, v) = 5, per half a node of omega children if omega > 1, per plaintext component a node of
    kappa children if kappa > 1, and kappa * omega element trees."""
    half = (5 if omega > 1 else 0) + omega * ((5 if kw > 1 else 0) + kw * element_bytes(curve, vb))
    return 5 + 2 * half


def component_offsets(curve, vb, kw, omega):
    """Where the 2 kappa omega element trees begin inside a ciphertext's bytes, in flat order (u half first, c = l kappa + j)."""
    E = element_bytes(curve, vb)
    out, at = [], 5
    for _ in range(2):
        at += 5 if omega > 1 else 0
        for _l in range(omega):
            at += 5 if kw > 1 else 0
            for _j in range(kw):
                out.append(at)
                at += E
    assert at == line_bytes(curve, vb, kw, omega)
    return out


# ---- trees -----------------------------------------------------------------------------------------------------------------------
def element_tree(curve, vb, el):
    if not curve:
        return leaf(int(el).to_bytes(vb, "big"))
    if el is None:
        return node([leaf(b"\xff" * vb), leaf(b"\xff" * vb)])
    return node([leaf(int(el[0]).to_bytes(vb, "big")), leaf(int(el[1]).to_bytes(vb, "big"))])


def array_tree(curve, vb, els):
    return node([element_tree(curve, vb, e) for e in els])


def ciphertext_tree(curve, vb, kw, row):
    """One ciphertext (a native line, F' of a commitment, a public key) given as its 2 kappa omega elements in flat order."""
    half = len(row) // 2
    trees = [element_tree(curve, vb, e) for e in row]
    return node([nest(trees[:half], kw), nest(trees[half:], kw)])


def native_text(curve, vb, kw, comps):
    """The native text of a list given as its 2 kappa omega component arrays (lists of elements)."""
    return b"".join(ciphertext_tree(curve, vb, kw, [c[i] for c in comps]).hex().encode("ascii") + b"\n" for i in range(len(comps[0])))


def list_tree(curve, vb, kw, comps):
    """A raw list file: node(U, V), each half the nested tree of its kappa omega component arrays."""
    half = len(comps) // 2
    trees = [array_tree(curve, vb, c) for c in comps]
    return node([nest(trees[:half], kw), nest(trees[half:], kw)])


def wide_array_tree(curve, vb, kw, comps):
    """An array of (G^kappa)^omega: DecryptionFactors%02d.bt, Plaintexts.bt."""
    return nest([array_tree(curve, vb, c) for c in comps], kw)


def ring_tree(xb, kw, values):
    """An element of (Z_q^kappa)^omega given as its kappa omega integers: k_F, the randomizers; kappa leaves under one node for
    Z_q^kappa (the decryption reply)."""
    return nest([leaf(int(v).to_bytes(xb, "big")) for v in values], kw)


def public_key_tree(curve, vb, kw, g, y):
    """FullPublicKey.bt: an element of getCiphPGroup(G^kappa, 1) = ((g, .., g), (y_0, .., y_(kappa-1)))  (:205-231)."""
    return ciphertext_tree(curve, vb, kw, [g] * kw + list(y))


def polynomial_tree(curve, vb, kw, coeffs):
    """PolynomialInExponent.bt: an array of `threshold` coefficients of G^kappa = node(kappa arrays), array j the rows j."""
    return nest([array_tree(curve, vb, [c[j] for c in coeffs]) for j in range(kw)], kw)


def commitment_tree(curve, vb, kw, yp, Bp):
    """DecrFactCommitment%02d.bt: node(y', B'), y' in G^kappa, B' in (G^kappa)^omega."""
    return node([nest([element_tree(curve, vb, e) for e in yp], kw), nest([element_tree(curve, vb, e) for e in Bp], kw)])


def reply_tree(xb, kw, kx):
    """DecrFactReply%02d.bt: k_x in Z_q^kappa."""
    return ring_tree(xb, kw, kx)


# ---- reading back (the tests open files with these) ---------------------------------------------------------------------------------
def decode(buf, pos=0):
    """(tree, next position): a leaf as bytes, a node as a list."""
    tag, n = buf[pos], int.from_bytes(buf[pos + 1:pos + 5], "big")
    pos += 5
    if tag == 1:
        return bytes(buf[pos:pos + n]), pos + n
    out = []
    for _ in range(n):
        t, pos = decode(buf, pos)
        out.append(t)
    return out, pos


def element_of(curve, tree):
    if not curve:
        return int.from_bytes(tree, "big")
    x, y = tree
    return None if set(x) == {0xff} and set(y) == {0xff} else (int.from_bytes(x, "big"), int.from_bytes(y, "big"))


def unnest(tree, kw, omega):
    """The kappa omega subtrees of a nested tree, in flat order."""
    comps = tree if omega > 1 else [tree]
    assert len(comps) == omega
    out = []
    for c in comps:
        rows = c if kw > 1 else [c]
        assert len(rows) == kw
        out += rows
    return out


def read_wide_array(curve, kw, omega, buf):
    tree, end = decode(buf)
    assert end == len(buf)
    return [[element_of(curve, e) for e in arr] for arr in unnest(tree, kw, omega)]


def read_list(curve, kw, omega, buf):
    tree, end = decode(buf)
    assert end == len(buf) and len(tree) == 2
    return [[element_of(curve, e) for e in arr] for half in tree for arr in unnest(half, kw, omega)]


# ---- the random oracle and what is derived with it (hvzk/ChallengerRO.java:96-116, PRGHeuristic) ----------------------------------
def random_oracle(rho, data, bits, hashname="sha256"):
    digest = hashlib.new(hashname, int(bits).to_bytes(4, "big") + rho + data).digest()
    out, ctr = bytearray(), 0
    while len(out) < (bits + 7) // 8:
        out += hashlib.new(hashname, digest + ctr.to_bytes(4, "big")).digest()
        ctr += 1
    out = out[:(bits + 7) // 8]
    if bits % 8:
        out[0] &= (1 << (bits % 8)) - 1
    return bytes(out)


def shuffle_seed(rho, g_tree, h_tree, u_tree, pk_tree, list_in, list_out, bits=256):
    """PoS.s / CCPoS.s: RO(rho, node(g, h, u, pk, w, w')) -- g, h, u of the atomic group, pk and the lists nested."""
    return random_oracle(rho, node([g_tree, h_tree, u_tree, pk_tree, list_in, list_out]), bits)


def decryption_seed(rho, curve, vb, kw, g, list_bytes, poly_bytes, factor_files, bits=256):
    """Dec.s: RO(rho, node(node(plainPGroup.getg(), ciphertexts), node(polynomial, node(factors of parties 1..k))))  (:1586-1607)"""
    g_tree = nest([element_tree(curve, vb, g)] * kw, kw)
    return random_oracle(rho, node([node([g_tree, list_bytes]), node([poly_bytes, node(list(factor_files))])]), bits)


def decryption_challenge(rho, seed, commitment_files, vbits):
    """Dec.v: RO(rho, node(leaf(seed), node(commitments of parties 1..k))) as a non-negative integer (:1624-1632)."""
    return int.from_bytes(random_oracle(rho, node([leaf(seed), node(list(commitment_files))]), vbits), "big")
