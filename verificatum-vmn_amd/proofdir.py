"""proofdir.py — the reference's proof directory ("nizkp") around one shuffle, written and verified by the C++ drivers.

The reference's standalone verifier reads everything it checks from files (``vmnv``):

    <nizkp>/Ciphertexts.bt                       the input list L_0       mixnet/MixNetElGamalSession.java:391-393
    <nizkp>/FullPublicKey.bt                     pk = (g, y)              (read by the verifier's readPublicKey)
    <nizkp>/proofs/PermutationCommitment%02d.bt  u of party l             hvzk/PoSTW.java:281-284
    <nizkp>/proofs/PoSCommitment%02d.bt          (B, A', B', C', D', F')  hvzk/PoSTW.java:293-296
    <nizkp>/proofs/PoSReply%02d.bt               (k_A, ..., k_F)          hvzk/PoSTW.java:305-307
    <nizkp>/proofs/Ciphertexts%02d.bt            the output list L_l      mixnet/ShufflerElGamalSession.java:1077-1079

``write_shuffle`` is what ``PoSTW.prove`` does with ``nizkp != null`` (hvzk/PoSTW.java:95-165: publish u, derive the seed of
the batching vector from node(g, h, u, pk, w, w'), commit, derive the challenge from node(leaf(seed), commitment), reply --
each message also written to its file); ``verify_shuffle`` is ``MixNetElGamalVerifyFiatShamirSession.verifyPoS``
(:843-937) including the values it prints under ``vmnv -t`` (``checkPrintTestVector``: der.rho, PoS.s, PoS.A, PoS.F, PoS.B,
PoS.Ap ... PoS.Fp, PoS.v, PoS.C, PoS.D, PoS.k_A ... PoS.k_F).  Both run the proof on the GPU through
``native.PoSBasicTW``; the hashing is hashlib on the host over the files' own bytes (they ARE the byte trees).

Above the single links: ``verify_session`` is the standalone verifier itself (MixNetElGamalVerifyFiatShamirSession.verify
:1318-1670 -- session files, keys, the chain of parties with its replacement rules, the decryption of the last list) and
``write_session`` plays all parties of a mixing, shuffling or decryption session; see the last part of this file.

What the reference takes from its protocol-info XML (session id, bit lengths, the descriptions of group / PRG / hash
that go into the global prefix, :158-189) is kept here in ``params.json`` next to the files; the XML itself and the
bulletin board are out of scope.

Under a public key of width kappa (``keywidth``; ProtocolElGamal.java:476-481, 738-744) the plaintext group is G^kappa
(MixNetElGamalVerifyFiatShamir.java:316-317) and a ciphertext of width omega has 2 kappa omega components, component
c = l kappa + j the key j of plaintext component l.  [NOT-IN-REF: VCR's PPGroup classes write the trees; here the rule of SURVEY.md
App. D -- a product element, array or ring element is the node of its factors' trees -- applied once more] every half of a list,
of a ciphertext-shaped element and every element of (Z_q^kappa)^omega is [omega > 1: node(omega; ...)] over [kappa > 1:
node(kappa; ...)] over the components' own trees (``fiatshamir.nested_tree``).  kappa = 1 leaves every byte as it was;
omega = 1 gives the bytes of an unkeyed list of width kappa.  The generators and der.rho do not depend on kappa (:556-576,
:158-189), and g in the seeds of the shuffles is the generator of the atomic group (:659, :769, :1483).  Everywhere below
``keywidth`` defaults to 1, ``width`` (where it is a parameter) is omega, and a wide key ``pkey`` has 2 kappa omega rows: g
repeated, then y_0 .. y_(kappa-1) repeated omega times.
"""
from __future__ import annotations

import dataclasses
import hashlib
import json
import os
import re
import shutil
import tempfile
import threading
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Sequence

from . import PGroupElementArray
from . import fiatshamir as fs
from . import native

PARAMS = "params.json"


def _p(nizkp: str, *names) -> str:
    return os.path.join(nizkp, *names)


def pc_file(nizkp, l):
    return _p(nizkp, "proofs", "PermutationCommitment%02d.bt" % l)          # PoSTW.PCfile :281-284


def posc_file(nizkp, l):
    return _p(nizkp, "proofs", "PoSCommitment%02d.bt" % l)                  # PoSTW.PoSCfile :293-296


def posr_file(nizkp, l):
    return _p(nizkp, "proofs", "PoSReply%02d.bt" % l)                       # PoSTW.PoSRfile :305-307


def l_file(nizkp, l):
    """The list party l reads: L_0 at the top of the directory, L_l below proofs/ (ShufflerElGamalSession.Lfile :1077-1079)."""
    return _p(nizkp, "Ciphertexts.bt") if l == 0 else _p(nizkp, "proofs", "Ciphertexts%02d.bt" % l)


def pk_file(nizkp):
    return _p(nizkp, "FullPublicKey.bt")


# ---- the global prefix and what is derived from it ----------------------------------------------------------------------
def global_prefix(params: dict) -> bytes:
    """``setGlobalPrefix`` (MixNetElGamalVerifyFiatShamirSession.java:158-189): rho = H(bytetree(node(version, sid.auxsid,
    n_r, n_v, n_e, s_PRG, s_Gq, s_H))) -- strings as leaves of their bytes, integers as 4-byte leaves."""
    s = lambda x: fs.leaf(x.encode("utf-8"))
    i = lambda x: fs.leaf(int(x).to_bytes(4, "big"))
    rosid = params["sid"] + "." + params["auxsid"]
    parts = [s(params["version"]), s(rosid), i(params["rbitlen"]), i(params["vbitlenro"]), i(params["ebitlenro"]),
             s(params["prg"]), s(params["pgroup"]), s(params["rohash"])]
    return hashlib.new(_hashname(params), fs._hdr(0, len(parts)) + b"".join(parts)).digest()


_HASHES = {"SHA-256": "sha256", "SHA-384": "sha384", "SHA-512": "sha512"}


def _hashname(params: dict) -> str:
    return _HASHES[params.get("rohash_name", "SHA-256")]


@dataclasses.dataclass(frozen=True)
class _Derived:
    """What the writers and verifiers below take from params.json: the bit lengths n_v, n_e, n_r, the random oracle's hash and
    its digest length in bits (the length of a shuffle's seed), rho with its challenger, and 8 * prg.minNoSeedBytes() -- the
    digest length of the PRG's hash function (PRGHeuristic), the length of the decryption's seed."""
    NV: int
    NE: int
    NR: int
    hashname: str
    bits: int
    rho: bytes
    chal: fs.Challenger
    prg: str

    @classmethod
    def of(cls, params: dict, rho: Optional[bytes] = None) -> "_Derived":
        hn = _hashname(params)
        rho = global_prefix(params) if rho is None else rho
        return cls(int(params["vbitlenro"]), int(params["ebitlenro"]), int(params["rbitlen"]), hn, 8 * hashlib.new(hn).digest_size,
                   rho, fs.Challenger(rho, hn), params.get("prg", "SHA-256"))

    @property
    def prg_bits(self) -> int:
        return 8 * hashlib.new(_HASHES[self.prg]).digest_size

    def seed(self, parts, bits: Optional[int] = None) -> bytes:
        """RO(rho || node(parts...)) of `bits` bits (default: a shuffle's): `parts` are the node's header with its first child,
        then the other children, hashed in order -- byte strings, or paths of files whose bytes are streamed in."""
        bits = self.bits if bits is None else bits
        d = self.chal.start(bits)
        for part in parts:
            if isinstance(part, str):
                with open(part, "rb") as f:
                    d.update(f.read())
            else:
                d.update(part)
        return self.chal.finish(d, bits)

    def challenge(self, seed: bytes, com_bt: bytes) -> int:
        """v = RO(rho || node(leaf(seed), commitment)) of n_v bits as a positive integer (PoSTW.java:141-149)."""
        return int.from_bytes(self.chal.challenge(fs._hdr(0, 2) + fs.leaf(seed) + com_bt, self.NV), "big")


def posc_seed_parts(g_tree: bytes, H_bt, u_bt) -> list:
    """node(g, h, u): the seed of a proof of a shuffle of commitments (PoSCTW.java:73-134; verifyPoSC :652-703)."""
    return [fs._hdr(0, 3) + g_tree, H_bt, u_bt]


def shuffle_seed_parts(g_tree: bytes, H_bt, u_bt, pk_tree: bytes, L, LP) -> list:
    """node(g, h, u, pk, L, L'): the seed of a proof of a shuffle, plain (PoSTW.java:114-129; verifyPoS :869-879) or
    commitment-consistent (CCPoSW.java:75-158).  A list may be given as the path of its file: the file IS its tree."""
    return [fs._hdr(0, 6) + g_tree, H_bt, u_bt, pk_tree, L, LP]


def derive_generators(grp, params: dict, rho: bytes, n: int) -> PGroupElementArray:
    """``IndependentGeneratorsRO("generators", H, rho, n_r).generate(pGroup, n)`` (distr/IndependentGeneratorsRO.java:110-130;
    called at MixNetElGamalVerifyFiatShamirSession.java:557-566): seed = RO(rho || leaf("generators")), then
    pGroup.randomElementArray(n, PRG(seed), n_r) on the GPU (vmn_garray_from_prg)."""
    D = _Derived.of(params, rho)
    return grp.elementArrayFromPRG(D.seed([fs.leaf(b"generators")]), n, D.NR)


# ---- arrays as files ------------------------------------------------------------------------------------------------------
def _nested_pieces(arrays: Sequence[PGroupElementArray], keywidth: int):
    """fs.nested_tree over the arrays' own trees, piece by piece (a list file is written without joining its arrays)."""
    if keywidth < 1 or len(arrays) % keywidth:
        raise ValueError("%d component arrays are no multiple of the key width %d" % (len(arrays), keywidth))
    omega = len(arrays) // keywidth
    if omega > 1:
        yield fs._hdr(0, omega)
    for l in range(omega):
        if keywidth > 1:
            yield fs._hdr(0, keywidth)
        for a in arrays[l * keywidth:(l + 1) * keywidth]:
            yield a.toByteTree()


def _list_pieces(comps: Sequence[PGroupElementArray], keywidth: int):
    """The bytes of a list file, piece by piece: node(u-part, v-part), each part nested."""
    half = len(comps) // 2
    yield fs._hdr(0, 2)
    for part in (comps[:half], comps[half:]):
        yield from _nested_pieces(part, keywidth)


def write_ciphertexts(path: str, comps: Sequence[PGroupElementArray], keywidth: int = 1) -> None:
    """A PPGroupElementArray of width w as 2w component arrays: node(u-part, v-part), a part being the array's own tree
    at width 1 and node(w array trees) otherwise; under a key of width kappa 2 kappa w arrays, a part
    nested once more (the head of this file)."""
    with open(path, "wb") as f:
        for piece in _list_pieces(comps, keywidth):
            f.write(piece)


def _ciphertexts_tree(comps: Sequence[PGroupElementArray], keywidth: int = 1) -> bytes:
    """The bytes write_ciphertexts puts into a list file."""
    return b"".join(_list_pieces(comps, keywidth))


def read_array_nests(grp, buf: bytes, nests: int, width: int, keywidth: int = 1, expected_n: int = 0):
    """THE reader of the arrays a file holds: `nests` nests (fs.nested_tree) of kappa * omega array trees each, under node(nests)
    where there is more than one, filling the whole of buf.  Every array has n elements: `expected_n`, or when that is 0 the
    count in the first array's own header; its bytes are cut out by grp.array_tree_size(n) and imported (range-checked) on the
    GPU.  No membership check: that is the caller's choice.  None when buf is no such tree or an import fails; the arrays
    imported until then are freed."""
    cur, comps, n = fs.Cursor(buf), [], expected_n or None

    def array(c):
        nonlocal n
        n = c.children() if n is None else n
        if c.children() != n:
            raise fs.NoSuchTree()
        comps.append(grp.toElementArrayFromByteTree(c.take(grp.array_tree_size(n)), n))
        return comps[-1]
    try:
        if nests > 1:
            cur.node(nests)
        for _ in range(nests):
            cur.nested(width, keywidth, array)
        cur.end()
        return comps
    except (fs.NoSuchTree, ValueError, native.VmnError):
        for a in comps:
            a.free()
        return None


def read_ciphertexts(grp, path: str, width: int, expected_n: int = 0, keywidth: int = 1) -> Optional[List[PGroupElementArray]]:
    """The 2w component arrays (2 kappa w under a key of width kappa) of a ciphertext list file, parsed (framing + range) on the
    GPU; None when the file is not such a list (the verifier then fails the party, :1446-1460).  Membership in the group is not
    checked here; interface.read_ciphertexts adds that check (_members_or_none)."""
    buf = _read_file(path)
    if buf is None:
        return None
    return parse_ciphertexts(grp, buf, width, expected_n, keywidth)


def parse_ciphertexts(grp, buf: bytes, width: int, expected_n: int = 0, keywidth: int = 1) -> Optional[List[PGroupElementArray]]:
    """read_ciphertexts for a list file whose bytes the caller already holds."""
    return read_array_nests(grp, buf, 2, width, keywidth, expected_n)


def _read_file(path: str) -> Optional[bytes]:
    """The bytes of a file of the directory; None when it is missing."""
    try:
        with open(path, "rb") as f:
            return f.read()
    except OSError:
        return None


def _write(path: str, data: bytes) -> bytes:
    """A file of the directory, written; hands the bytes back."""
    with open(path, "wb") as f:
        f.write(data)
    return data


def _hex(x) -> str:
    """A group element / ring element as text: hexadecimal for integers, (x, y) in hexadecimal for curve points.  VCR's own
    toString() of these objects is not part of the reference tree: a maintainer who diffs against `vmnv -t` compares VALUES."""
    if x is None:
        return "INFINITY"
    if isinstance(x, tuple):
        return "(" + ", ".join(format(int(c), "x") for c in x) + ")"
    return format(int(x), "x")


def _hexes(xs) -> str:
    """A tuple of elements as text: "(_hex(x_0), _hex(x_1), ..)"."""
    return "(" + ", ".join(_hex(x) for x in xs) + ")"


def _arr(a) -> str:
    return _hexes(a.toInts())


def _hexk(x, keywidth: int = 1) -> str:
    """_hex for an element of G^kappa resp. Z_q^kappa given as its kappa rows: "(row_0, .., row_(kappa-1))", the row itself at kappa = 1."""
    return _hex(x) if keywidth == 1 else _hexes(x)


# ---- prover: PoSTW.prove with nizkp != null ----------------------------------------------------------------------------
def write_shuffle(nizkp: str, l: int, grp, params: dict, pkey: Sequence, W: Sequence[PGroupElementArray], rand,
                  H: Optional[PGroupElementArray] = None, out_file: Optional[str] = None, keywidth: int = 1) -> List[PGroupElementArray]:
    """Party l shuffles the list in l_file(nizkp, l - 1) (given as W) and proves it: re-encryption + permutation
    (ShufflerElGamalSession.java:400-409, 273-278), then PoSTW.prove (:95-165).  Returns w'; writes L_l and the three
    proof files.  `rand`: the prover's random source (native.RandomSource semantics).  `out_file`: where L_l goes instead of
    l_file(nizkp, l) (a session's last list, write_session)."""
    out_file = out_file or l_file(nizkp, l)
    os.makedirs(_p(nizkp, "proofs"), exist_ok=True)
    D = _Derived.of(params)
    n, width = W[0].size(), len(W) // 2
    own_h = H is None
    if own_h:
        H = derive_generators(grp, params, D.rho, n)
    g = grp.g
    pi = rand.permutation(n)
    S = [native.random_ring_array_native(grp, rand, n, D.NR) for _ in range(width)]
    prover = native.PoSBasicTW(grp, D.NV, D.NE, D.NR, rand=rand)
    prover.precompute(g, H, pi)
    WP = native.reencrypt_native(grp, pkey, W, S, pi)
    write_ciphertexts(out_file, WP, keywidth)                                    # (before the seed, which is hashed over the file)
    prover.setInstance(pkey, W, WP, S)
    u_bt = _write(pc_file(nizkp, l), prover.u.toByteTree())                      # "PermutationCommitment" :107-112
    box = {}

    def commit(seed):                                                            # the seed of the batching vector :114-129
        prover.setBatchVectorSeed(seed)
        box["com"] = prover.commit()
        return _write(posc_file(nizkp, l), _keyed(box["com"].native, keywidth).toByteTree())      # "Commitment" :131-139
    parts = shuffle_seed_parts(grp.element_tree(g), H.toByteTree(), u_bt, fs.product_element_tree(grp, pkey, keywidth),
                               l_file(nizkp, l - 1), out_file)
    rep = prover.reply(_seed_and_challenge(D, parts, commit))                    # :141-149
    _write(posr_file(nizkp, l), _keyed(rep.native, keywidth).toByteTree())       # "Reply" :151-159
    box.clear()
    rep = None
    prover.free()
    for a in S:
        a.free()
    if own_h:
        H.free()
    return WP


def _keyed(msg, keywidth: int):
    """The proof message `msg` (native.Message), written under the key width from now on."""
    return msg if keywidth == 1 else msg.setKeyWidth(keywidth)


def write_inputs(nizkp: str, grp, params: dict, pkey: Sequence, W: Sequence[PGroupElementArray], keywidth: int = 1) -> None:
    """params.json, FullPublicKey.bt and the input list L_0.  `pkey`: the rows of the key as the file holds it -- for a session
    the basic key (g, .., g, y_0, .., y_(kappa-1)), an element of getCiphPGroup(plainPGroup, 1)."""
    os.makedirs(_p(nizkp, "proofs"), exist_ok=True)
    with open(_p(nizkp, PARAMS), "w") as f:
        json.dump(params, f, indent=1)
    _write(pk_file(nizkp), fs.product_element_tree(grp, pkey, keywidth))
    write_ciphertexts(l_file(nizkp, 0), W, keywidth)


# ---- verifier: MixNetElGamalVerifyFiatShamirSession.verifyPoS -----------------------------------------------------------
def verify_shuffle(nizkp: str, l: int, grp, params: dict, pkey: Sequence, vectors: Optional[Dict[str, str]] = None,
                   with_arrays: bool = False, keywidth: int = 1) -> bool:
    """verifyPoS(l, g, generators, input = L_(l-1), output = L_l) (:843-937).  `vectors` (a dict) receives the test vectors
    the reference prints under `vmnv -t` at the places it prints them; `with_arrays` adds the N-sized ones (PoS.B, PoS.Bp,
    PoS.k_B, PoS.k_E, bas.h).  A file that cannot be parsed makes the verdict False (the reference substitutes trivial values
    and the equations then fail)."""
    tv = vectors if vectors is not None else {}
    width = len(pkey) // 2 // keywidth
    D = _Derived.of(params)
    tv["der.rho"] = D.rho.hex()                                                # :188
    W = read_ciphertexts(grp, l_file(nizkp, l - 1), width, 0, keywidth)
    if W is None:
        return False
    n = W[0].size()
    WP = read_ciphertexts(grp, l_file(nizkp, l), width, n, keywidth)
    if WP is None:
        return False
    H = derive_generators(grp, params, D.rho, n)                               # :557-566
    if with_arrays:
        tv["bas.h"] = _arr(H)
    u_bt = _read_file(pc_file(nizkp, l))                                       # :861-866
    U = parse_commitment(grp, u_bt, n)
    if U is None:
        return False
    seed = lambda: D.seed(shuffle_seed_parts(grp.element_tree(grp.g), H.toByteTree(), u_bt,                  # :869-879
                                             fs.product_element_tree(grp, pkey, keywidth), l_file(nizkp, l - 1), l_file(nizkp, l)))
    verdict = pos_core(nizkp, l, grp, params, pkey, W, WP, H, U, seed, tv, with_arrays, keywidth)
    for a in W + WP + [H, U]:
        a.free()
    return verdict


def parse_commitment(grp, u_bt: Optional[bytes], n: int) -> Optional[PGroupElementArray]:
    """The permutation commitment of a PermutationCommitment%02d.bt file's bytes: n elements of the group; None when the file
    is missing or is no such array."""
    try:
        if u_bt is None:
            raise ValueError("no permutation commitment")
        U = grp.toElementArrayFromByteTree(u_bt, n)
        if not U.isMember():
            raise ValueError("u outside the group")
        return U
    except (ValueError, native.VmnError):
        return None


def pos_core(nizkp: str, l: int, grp, params: dict, pkey: Sequence, W, WP, H, U, seed, tv: dict, with_arrays: bool = False,
             keywidth: int = 1) -> bool:
    """verifyPoS on loaded inputs: the lists W and WP, the generators H and the permutation commitment U as device arrays,
    `seed()` -> the seed of the batching vector (the one value that depends on the lists' and the generators' BYTES).  Reads
    the party's commitment and reply files; frees nothing it was given."""
    D = _Derived.of(params)
    n, width = W[0].size(), len(pkey) // 2
    V = native.PoSBasicTW(grp, D.NV, D.NE, D.NR)
    try:
        V.precompute(grp.g, H)                                                     # :857
        V.setInstance(pkey, W, WP)
        V.setPermutationCommitment(U)
        seed = seed()
        tv["PoS.s"] = seed.hex()                                                   # :881
        V.setBatchVectorSeed(seed)                                                 # :883
        V.computeAF()                                                              # :886
        tv["PoS.A"], tv["PoS.F"] = _hex(V.getA()), _hexes(V.getF())                # :888-889
        com_bt = _read_file(posc_file(nizkp, l))                                   # :892-895
        com = V.readCommitment(com_bt, n, width, keywidth) if com_bt is not None else None
        if com is None:
            return False
        V.setCommitment(com)
        if with_arrays:                                                            # :897-902
            tv["PoS.B"], tv["PoS.Bp"] = _arr(com.item(0)), _arr(com.item(2))
        tv["PoS.Ap"], tv["PoS.Cp"], tv["PoS.Dp"] = (_hex(com.item(k)[0]) for k in (1, 3, 4))
        tv["PoS.Fp"] = _hexes(com.item(5))
        vch = D.challenge(seed, com_bt)                                            # :905-913
        tv["PoS.v"] = format(vch, "x")                                             # :915
        V.setChallenge(vch)
        rep_bt = _read_file(posr_file(nizkp, l))                                   # :921-925
        rep = V.readReply(rep_bt, n, width, keywidth) if rep_bt is not None else None
        if rep is None:
            return False
        verdict = V.verify(rep)
        tv["PoS.C"], tv["PoS.D"] = _hex(V.getC()), _hex(V.getD())                  # :927-928
        tv["PoS.k_A"], tv["PoS.k_C"], tv["PoS.k_D"] = (_hex(rep.item(k)[0]) for k in (0, 2, 3))      # :930-934
        tv["PoS.k_F"] = _hexes(rep.item(5))
        if with_arrays:
            tv["PoS.k_B"], tv["PoS.k_E"] = _arr(rep.item(1)), _arr(rep.item(4))
        tv["verdicts(A,B,C,D,F)"] = str(V.verdicts)
        return bool(verdict)
    finally:
        V.free()


# =============================================================================================================================
# The precomputed shuffle: permutation commitment + PoSC offline, shrink + re-encryption + CCPoS online (BASELINE configs[2], [4])
#     <nizkp>/proofs/PermutationCommitment%02d.bt   u for N_0 ciphertexts     mixnet/PermutationCommitment.java:228-230, 364
#     <nizkp>/proofs/PoSCCommitment%02d.bt, PoSCReply%02d.bt                  hvzk/PoSCTW.java:221-235
#     <nizkp>/proofs/KeepList%02d.bt                the positions kept for N  mixnet/PermutationCommitment.java:240-242, 413, 455
#     <nizkp>/proofs/CCPoSCommitment%02d.bt, CCPoSReply%02d.bt                hvzk/CCPoSW.java:274-288
#     <nizkp>/proofs/Ciphertexts%02d.bt             the output list
# Prover: PermutationCommitment.generate :251-366 + PoSCTW.prove :73-134; shrink :390-471; ShufflerElGamalSession committed
# shuffle :789-792 + CCPoSW.prove :75-158.  Verifier: readPermutationCommitment :618-636, verifyPoSC :652-703, shrinkPermComm
# :714-746, verifyCCPoS :757-830 of MixNetElGamalVerifyFiatShamirSession.java.
# =============================================================================================================================
def poscc_file(nizkp, l):
    return _p(nizkp, "proofs", "PoSCCommitment%02d.bt" % l)


def poscr_file(nizkp, l):
    return _p(nizkp, "proofs", "PoSCReply%02d.bt" % l)


def kl_file(nizkp, l):
    return _p(nizkp, "proofs", "KeepList%02d.bt" % l)


def ccposc_file(nizkp, l):
    return _p(nizkp, "proofs", "CCPoSCommitment%02d.bt" % l)


def ccposr_file(nizkp, l):
    return _p(nizkp, "proofs", "CCPoSReply%02d.bt" % l)


def _booleans_tree(flags) -> bytes:
    """A boolean array as a byte tree: one leaf, one byte per flag (ByteTree.booleanArrayToByteTree is VCR code, not in the
    reference tree: [NOT-IN-REF], restated from the verifier specification)."""
    return fs.leaf(bytes(1 if f else 0 for f in flags))


def _parse_booleans(buf: Optional[bytes], n: int):
    """The n flags of a boolean array's bytes; None when there are none or they are no such leaf."""
    try:
        if buf is None:
            return None
        cur = fs.Cursor(buf)
        data = cur.leaf(n)
        cur.end()
        return None if any(b > 1 for b in data) else [b == 1 for b in data]
    except fs.NoSuchTree:
        return None


def _read_booleans(path: str, n: int):
    return _parse_booleans(_read_file(path), n)


def _seed_and_challenge(D: _Derived, parts, commit_fn) -> int:
    """A prover's two random-oracle calls around its commitment: seed = D.seed(parts), commit_fn(seed) -> the bytes of the
    commitment it publishes, v = D.challenge(seed, those bytes)."""
    seed = D.seed(parts)
    return D.challenge(seed, commit_fn(seed))


def write_precomputation(nizkp: str, l: int, grp, params: dict, n_max: int, rand, H: Optional[PGroupElementArray] = None,
                         keywidth: int = 1):
    """`vmn -precomp` of party l for N_0 = n_max ciphertexts: the permutation commitment u and its proof of a shuffle of
    commitments.  Returns the prover's secrets for the online phase: (pi, R, U, H).  Nothing here depends on `keywidth`: the
    commitment and its proof live in the atomic group (:652-703); the parameter is what write_session hands every writer."""
    os.makedirs(_p(nizkp, "proofs"), exist_ok=True)
    D = _Derived.of(params)
    if H is None:
        H = derive_generators(grp, params, D.rho, n_max)
    g = grp.g
    pi = rand.permutation(n_max)
    R = native.random_ring_array_native(grp, rand, n_max, D.NR)
    U = native.permutation_commitment_native(grp, g, H, R, pi)
    u_bt = _write(pc_file(nizkp, l), U.toByteTree())                             # PermutationCommitment.java:364
    P = native.PoSCBasicTW(grp, D.NV, D.NE, D.NR, rand=rand)                     # PoSCTW.prove :73-134
    P.setInstance(g, H, U, R, pi)
    box = {}

    def commit(seed):
        P.setBatchVectorSeed(seed)
        box["com"] = P.commit()
        return _write(poscc_file(nizkp, l), box["com"].native.toByteTree())
    rep = P.reply(_seed_and_challenge(D, posc_seed_parts(grp.element_tree(g), H.toByteTree(), u_bt), commit))
    _write(poscr_file(nizkp, l), rep.native.toByteTree())
    box.clear()
    rep = None
    P.free()
    return pi, R, U, H


def write_committed_shuffle(nizkp: str, l: int, grp, params: dict, pkey: Sequence, W: Sequence[PGroupElementArray], rand,
                            pi, R, U, H, out_file: Optional[str] = None, keywidth: int = 1) -> List[PGroupElementArray]:
    """The online phase for the N <= N_0 ciphertexts that arrived (W = the list in l_file(nizkp, l - 1)): shrink
    (PermutationCommitment.java:390-471, keep list to its file), re-encrypt and permute (ShufflerElGamalSession.java:789-792),
    CCPoSW.prove (:75-158).  Returns w'.  `out_file`: where L_l goes instead of l_file(nizkp, l)."""
    out_file = out_file or l_file(nizkp, l)
    D = _Derived.of(params)
    n, width = W[0].size(), len(W) // 2
    g = grp.g
    keep, pi_s = native.permutation_shrink_native(pi, n)
    _write(kl_file(nizkp, l), _booleans_tree(keep))
    U_s, R_s, H_s = U.extract(keep), R.copyOfRange(0, n), H.copyOfRange(0, n)
    S = [native.random_ring_array_native(grp, rand, n, D.NR) for _ in range(width)]
    WP = native.reencrypt_native(grp, pkey, W, S, pi_s)
    write_ciphertexts(out_file, WP, keywidth)
    P = native.CCPoSBasicW(grp, D.NV, D.NE, D.NR, rand=rand)
    P.setInstance(g, H_s, U_s, pkey, W, WP, R_s, pi_s, S)
    box = {}

    def commit(seed):
        P.setBatchVectorSeed(seed)
        box["com"] = P.commit()
        return _write(ccposc_file(nizkp, l), _keyed(box["com"].native, keywidth).toByteTree())
    parts = shuffle_seed_parts(grp.element_tree(g), H_s.toByteTree(), U_s.toByteTree(), fs.product_element_tree(grp, pkey, keywidth),
                               l_file(nizkp, l - 1), out_file)
    rep = P.reply(_seed_and_challenge(D, parts, commit))
    _write(ccposr_file(nizkp, l), _keyed(rep.native, keywidth).toByteTree())
    box.clear()
    rep = None
    P.free()
    for a in S + [U_s, R_s, H_s]:
        a.free()
    return WP


def verify_precomputed_shuffle(nizkp: str, l: int, grp, params: dict, pkey: Sequence, n_max: int,
                               vectors: Optional[Dict[str, str]] = None, keywidth: int = 1) -> bool:
    """The standalone verifier's path for a precomputed shuffle of party l (MixNetElGamalVerifyFiatShamirSession.java
    :1395-1500): readPermutationCommitment(N_0), verifyPoSC, read the output, shrinkPermComm through the keep list, verifyCCPoS.
    `vectors` receives der.rho, PoSC.s, PoSC.v, CCPoS.s, CCPoS.v (the names the reference registers, Tool.java:155-175) and the
    verifiers' intermediates (PoSC.A/C/D, CCPoS.A, CCPoS.B: not printed by the reference; for diffing two builds of this code)."""
    tv = vectors if vectors is not None else {}
    width = len(pkey) // 2 // keywidth
    D = _Derived.of(params)
    tv["der.rho"] = D.rho.hex()
    g_tree = grp.element_tree(grp.g)
    H = derive_generators(grp, params, D.rho, n_max)
    u_bt = _read_file(pc_file(nizkp, l))                                         # readPermutationCommitment :618-636
    U = parse_commitment(grp, u_bt, n_max)
    if U is None:
        return False
    if not posc_core(nizkp, l, grp, params, H, U, n_max, lambda: D.seed(posc_seed_parts(g_tree, H.toByteTree(), u_bt)), tv):
        return False           # (the reference then takes the generators for u and goes on; a harness stops with the verdict)
    # ---- the lists, the keep list, verifyCCPoS :757-830
    W = read_ciphertexts(grp, l_file(nizkp, l - 1), width, 0, keywidth)
    if W is None:
        return False
    n = W[0].size()
    WP = read_ciphertexts(grp, l_file(nizkp, l), width, n, keywidth)
    if WP is None:
        return False
    keep = read_keep_list(nizkp, l, n_max, n)
    if keep is None:                                                             # shrinkPermComm :714-746 fails the party
        return False
    U_s, H_s = U.extract(keep), H.copyOfRange(0, n)
    seed2 = lambda: D.seed(shuffle_seed_parts(g_tree, H_s.toByteTree(), U_s.toByteTree(), fs.product_element_tree(grp, pkey, keywidth),
                                              l_file(nizkp, l - 1), l_file(nizkp, l)))
    verdict = ccpos_core(nizkp, l, grp, params, pkey, H_s, U_s, W, WP, seed2, tv, keywidth)
    for a in W + WP + [H, U, U_s, H_s]:
        a.free()
    return verdict


def read_keep_list(nizkp: str, l: int, n_max: int, n: int):
    """The keep list of party l: n_max booleans of which n are set; None when the file is missing or is no such list."""
    keep = _read_booleans(kl_file(nizkp, l), n_max)
    return keep if keep is not None and sum(keep) == n else None


def _read_message(grp, path: str, kinds, sizes, keywidth: int = 1):
    """(the bytes of a proof message's file, the message); (None, None) when the file is missing, (bytes, None) when its
    bytes are no such message."""
    bt = _read_file(path)
    return bt, (native.Message.fromByteTree(grp, bt, kinds, sizes, keywidth) if bt is not None else None)


def posc_core(nizkp: str, l: int, grp, params: dict, H, U, n_max: int, seed, tv: dict) -> bool:
    """verifyPoSC (:652-703) on loaded inputs: the generators H and the permutation commitment U (n_max elements each) as device
    arrays, `seed()` -> the seed of the batching vector.  Frees nothing it was given."""
    D = _Derived.of(params)
    V = native.PoSCBasicTW(grp, D.NV, D.NE, D.NR)
    try:
        V.setInstance(grp.g, H, U)
        seed = seed()
        tv["PoSC.s"] = seed.hex()
        V.setBatchVectorSeed(seed)
        com_bt, com = _read_message(grp, poscc_file(nizkp, l), native.PoSCBasicTW._com_kinds, [n_max, 1, n_max, 1, 1])
        if com is None:
            return False
        V.setCommitment(com)
        v = D.challenge(seed, com_bt)
        tv["PoSC.v"] = format(v, "x")
        V.setChallenge(v)
        _, rep = _read_message(grp, poscr_file(nizkp, l), native.PoSCBasicTW._rep_kinds, [1, n_max, 1, 1, n_max])
        if rep is None:
            return False
        ok_posc = V.verify(rep)
        tv["PoSC.A"], tv["PoSC.C"], tv["PoSC.D"] = _hex(V.getA()), _hex(V.getC()), _hex(V.getD())
        return bool(ok_posc)
    finally:
        V.free()


def ccpos_core(nizkp: str, l: int, grp, params: dict, pkey: Sequence, H_s, U_s, W, WP, seed, tv: dict, keywidth: int = 1) -> bool:
    """verifyCCPoS (:757-830) on loaded inputs: the shrunk generators and permutation commitment and the two lists as device
    arrays, `seed()` -> the seed of the batching vector.  Frees nothing it was given."""
    D = _Derived.of(params)
    n, width = W[0].size(), len(pkey) // 2
    C = native.CCPoSBasicW(grp, D.NV, D.NE, D.NR)
    try:
        C.setInstance(grp.g, H_s, U_s, pkey, W, WP)
        seed2 = seed()
        tv["CCPoS.s"] = seed2.hex()
        C.setBatchVectorSeed(seed2)
        C.computeAB()
        A, B = C.getAB()
        tv["CCPoS.A"], tv["CCPoS.B"] = _hex(A), _hexes(B)
        com_bt, com = _read_message(grp, ccposc_file(nizkp, l), native.CCPoSBasicW._com_kinds, [1, 2 * width], keywidth)
        if com is None:
            return False
        C.setCommitment(com)
        v2 = D.challenge(seed2, com_bt)
        tv["CCPoS.v"] = format(v2, "x")
        C.setChallenge(v2)
        _, rep = _read_message(grp, ccposr_file(nizkp, l), native.CCPoSBasicW._rep_kinds, [1, width, n], keywidth)
        if rep is None:
            return False
        return bool(C.verify(rep))
    finally:
        C.free()


# =============================================================================================================================
# Verifiable threshold decryption of the last list (row A6), widths >= 1 over a modular group or a curve
#     <nizkp>/proofs/PolynomialInExponent.bt      the coefficients g^(a_d) of the key's polynomial in the exponent
#     <nizkp>/proofs/DecryptionFactors%02d.bt     f_l = u^(-x_l / c) of party l     elgamal/DistrElGamalSession.java:574-577
#     <nizkp>/proofs/DecrFactCommitment%02d.bt    node(y'_l, B'_l)                  :586-589
#     <nizkp>/proofs/DecrFactReply%02d.bt         k_x,l                             :598-601
#     <nizkp>/proofs/CorrectIndices.bt            k + 1 booleans (entry 0 unused)   :553-555
#     <nizkp>/Plaintexts.bt                       second components x combined factors   mixnet/MixNetElGamalSession.java:413
# Prover side: DistrElGamalSession.decrypt (:344-545) with every party played here; verifier: the decryption branch of
# MixNetElGamalVerifyFiatShamirSession.verify (:1545-1667, helpers :1098-1297).  An array of G^omega (the factors, the plaintexts)
# is node(omega array trees), the array's own tree at omega = 1 -- a part of a ciphertext list file; an element of G^omega (B')
# is node(omega element trees), the element's own tree at omega = 1.  An element's tree is a leaf over a modular group and
# node(leaf(x), leaf(y)) over a curve (infinity: both leaves 0xff), as in the arrays and messages the library writes.
# Under a key of width kappa (v.plainPGroup = G^kappa) the factors, the plaintexts and B' are nested once more (the head of this
# file); y' is node(kappa element trees), the reply node(kappa leaves) (Z_q^kappa), the polynomial in the exponent -- threshold
# coefficients in G^kappa, :239-265 -- node(kappa array trees), array j holding row j of every coefficient; a key, a share and a
# coefficient are then kappa-tuples, row 0 first.
# =============================================================================================================================
def poly_file(nizkp):
    return _p(nizkp, "proofs", "PolynomialInExponent.bt")


def df_file(nizkp, l):
    return _p(nizkp, "proofs", "DecryptionFactors%02d.bt" % l)


def dfc_file(nizkp, l):
    return _p(nizkp, "proofs", "DecrFactCommitment%02d.bt" % l)


def dfr_file(nizkp, l):
    return _p(nizkp, "proofs", "DecrFactReply%02d.bt" % l)


def cr_file(nizkp):
    return _p(nizkp, "proofs", "CorrectIndices.bt")


def plaintexts_file(nizkp):
    return _p(nizkp, "Plaintexts.bt")


def _wide_array_tree(comps: Sequence[PGroupElementArray], keywidth: int = 1) -> bytes:
    """toByteTree() of an array of G^omega given as its omega component arrays, of (G^kappa)^omega given as its kappa omega."""
    return fs.nested_tree([a.toByteTree() for a in comps], keywidth)


def _member_arrays(comps):
    """comps when every array lies in the group; else -- also when the check itself fails -- None, and the arrays are freed."""
    if comps is None:
        return None
    try:
        if all(c.isMember() for c in comps):
            return comps
    except (ValueError, native.VmnError):
        pass
    for c in comps:
        c.free()
    return None


def _read_wide_array(grp, path: str, width: int, n: int, keywidth: int = 1) -> Optional[List[PGroupElementArray]]:
    """The omega component arrays (kappa omega under a key of width kappa; n elements each) of such a file; None when the file
    is missing or is no such array."""
    buf = _read_file(path)
    return _member_arrays(read_array_nests(grp, buf, 1, width, keywidth, n)) if buf is not None else None


def _rows(x, keywidth: int):
    """An element of G^kappa / Z_q^kappa as the tuple of its rows (kappa = 1: the element itself is the one row)."""
    return (x,) if keywidth == 1 else tuple(x)


def _unrows(rows, keywidth: int):
    """_rows back: the one row itself at kappa = 1, the tuple of the rows otherwise."""
    return rows[0] if keywidth == 1 else tuple(rows)


def _y_rows(pkey: Sequence, width: int, keywidth: int):
    """y of a wide key of 2 * width rows (g repeated, then y_0 .. y_(kappa-1) repeated omega times): the element at kappa = 1,
    else its kappa rows."""
    return pkey[-1] if keywidth == 1 else tuple(pkey[width:width + keywidth])


def _commitment_tree(grp, yp, Bp, keywidth: int = 1) -> bytes:
    return fs._hdr(0, 2) + fs.nested_tree([grp.element_tree(e) for e in _rows(yp, keywidth)], keywidth) + fs.wide_element_tree(grp, Bp, keywidth)


def _reply_tree(grp, kx, keywidth: int = 1) -> bytes:
    """k_x of Z_q^kappa: node(kappa leaves), the leaf itself at kappa = 1."""
    return fs.nested_tree([fs.leaf(int(v).to_bytes(grp.exp_bytes, "big")) for v in _rows(kx, keywidth)], keywidth)


def _read_reply(grp, buf: bytes, keywidth: int = 1):
    """The reply of a DecrFactReply file's bytes (an integer, a kappa-tuple under a key of width kappa); None when the bytes are
    no such tree.  A row >= q is handed on: it costs the party its verdict, not the file its format (:606-613)."""
    try:
        cur = fs.Cursor(buf)
        rows = cur.nested(1, keywidth, lambda c: int.from_bytes(c.leaf(grp.exp_bytes), "big"))
        cur.end()
        return _unrows(rows, keywidth)
    except fs.NoSuchTree:
        return None


def _read_element_nests(grp, buf: Optional[bytes], widths: Sequence[int], keywidth: int):
    """node(len(widths) nests) filling buf, nest i holding kappa * widths[i] element trees: the nests' elements, or None when
    there are no bytes or the framing is wrong (over a curve also: a leaf that is not of the coordinate width, a point that is
    not on the curve)."""
    try:
        if buf is None:
            return None
        cur = fs.Cursor(buf)
        cur.node(len(widths))
        nests = [cur.nested(w, keywidth, lambda c: c.item(grp.element_from_tree)) for w in widths]
        cur.end()
        return nests
    except fs.NoSuchTree:
        return None


def _read_commitment(grp, path: str, width: int, keywidth: int = 1):
    """(y', (B'_0 .. B'_(omega-1))) of a commitment file as group elements (y' a kappa-tuple and B' kappa omega elements under a
    key of width kappa); None when the file is missing or is no such tree."""
    got = _read_element_nests(grp, _read_file(path), (1, width), keywidth)
    return (_unrows(got[0], keywidth), tuple(got[1])) if got is not None else None


def eval_polynomial_in_exponent(grp, coeffs: Sequence, l: int):
    """y_l = prod_d coeffs[d]^(l^d): the public key share of party l (PolynomialInExponent.evaluate)."""
    acc, power = grp.ONE, 1
    for c in coeffs:
        acc = grp.k_mul(acc, grp.k_exp(c, power))
        power = power * l % grp.q
    return acc


def eval_keys(grp, coeffs: Sequence, l: int, keywidth: int = 1):
    """eval_polynomial_in_exponent row by row for coefficients in G^kappa (kappa-tuples): the kappa-tuple y_l."""
    if keywidth == 1:
        return eval_polynomial_in_exponent(grp, coeffs, l)
    return tuple(eval_polynomial_in_exponent(grp, [c[j] for c in coeffs], l) for j in range(keywidth))


def _polynomial_tree(grp, poly: Sequence, keywidth: int = 1) -> bytes:
    """PolynomialInExponent.bt: the array tree of the coefficients; in G^kappa node(kappa array trees), array j = row j."""
    arrays = [grp.toElementArray([_rows(c, keywidth)[j] for c in poly]) for j in range(keywidth)]
    bt = fs.nested_tree([a.toByteTree() for a in arrays], keywidth)
    for a in arrays:
        a.free()
    return bt


def parse_polynomial(grp, buf: Optional[bytes], threshold: int, keywidth: int = 1):
    """The `threshold` coefficients of a PolynomialInExponent.bt file's bytes (kappa-tuples under a key of width kappa); None
    when the bytes are no such tree or a coefficient is outside the group."""
    arrays = _member_arrays(read_array_nests(grp, buf, 1, 1, keywidth, threshold)) if buf is not None else None
    if arrays is None:
        return None
    try:
        rows = [a.toInts() for a in arrays]
        return rows[0] if keywidth == 1 else [tuple(r[d] for r in rows) for d in range(threshold)]
    except (ValueError, native.VmnError):
        return None
    finally:
        for a in arrays:
            a.free()


def _decryption_seed(D: _Derived, grp, list_bytes: bytes, poly_bt: bytes, factors: Sequence, keywidth: int = 1) -> bytes:
    """challenge(node(node(g, ciphertexts), node(polynomial, node(factors of parties 1..k))), 8 * minNoSeedBytes)  :434-461;
    g is plainPGroup.getg() = (g, .., g) (:1587).  `factors`: every party's factors as device arrays."""
    head = fs._hdr(0, 2) + fs._hdr(0, 2) + fs.nested_tree([grp.element_tree(grp.g)] * keywidth, keywidth)
    trees = [_wide_array_tree(fl, keywidth) for fl in factors]
    return D.seed([head, list_bytes, fs._hdr(0, 2) + poly_bt + fs._hdr(0, len(trees))] + trees, D.prg_bits)


def write_decryption(nizkp: str, grp, params: dict, pkey: Sequence, W: Sequence[PGroupElementArray], poly: Sequence[int],
                     shares: Sequence[Optional[int]], rand, k: int, threshold: int,
                     tamper=None, keywidth: int = 1, tamper_reply=None) -> List[PGroupElementArray]:
    """All k parties of DistrElGamalSession.decrypt (:344-545) on the list W (2 omega component arrays, the list the last mix
    server wrote): `poly` = the coefficients g^(a_d) of the polynomial in the exponent (threshold of them), `shares` = the
    secret shares x_l (k + 1 entries, entry 0 unused), `rand` = the parties' random source.  Writes the six kinds of files and
    returns the plaintexts (omega arrays).  The polynomial in the exponent is written as the array tree of its coefficients:
    PGroup.toByteTree(PGroupElement[]) is VCR code, not part of the reference tree.  `tamper(l, factors)` (tests): replaces the
    factors party l publishes; `tamper_reply(l, k_x)` (tests): the reply it publishes.  Under a key of width `keywidth` = kappa
    W has 2 kappa omega arrays and a coefficient of `poly` and a share are kappa-tuples."""
    os.makedirs(_p(nizkp, "proofs"), exist_ok=True)
    D = _Derived.of(params)
    width = len(W) // 2                                                            # components in all: kappa * omega
    U, V = list(W[:width]), list(W[width:])
    y = _y_rows(pkey, width, keywidth)
    keyed = {} if keywidth == 1 else {"keywidth": keywidth}
    ys = [None] + [eval_keys(grp, poly, l, keywidth) for l in range(1, k + 1)]
    poly_bt = _write(poly_file(nizkp), _polynomial_tree(grp, poly, keywidth))
    F: List[Optional[List[PGroupElementArray]]] = [None]
    for l in range(1, k + 1):                                                      # :384-399
        fl = native.decryptionFactors(U, shares[l] if keywidth == 1 else list(shares[l]), grp.q, k)
        if tamper is not None:
            fl = tamper(l, fl)
        F.append(fl)
        _write(df_file(nizkp, l), _wide_array_tree(fl, keywidth))
    correct = [True] * (k + 1)
    comb = native.combineDecryptionFactors(F, correct, k, threshold, grp.q)         # :406-410
    seed = _decryption_seed(D, grp, _ciphertexts_tree(W, keywidth), poly_bt, F[1:], keywidth)
    sessions = []
    for l in range(1, k + 1):
        s = native.DistrElGamalSessionBasic(grp, l, k, threshold, D.NE, rand=rand)
        s.setInstance(U, ys, F, **keyed)
        s.setBatchVectorSeed(seed)
        s.batchInput()
        sessions.append(s)
    commitments, trees = [None], []
    for l in range(1, k + 1):                                                      # :469
        commitments.append(sessions[l - 1].commit(shares[l]))
        trees.append(_write(dfc_file(nizkp, l), _commitment_tree(grp, *commitments[l], keywidth)))
    v = D.challenge(seed, fs._hdr(0, k) + b"".join(trees))                         # :474-480
    ver = sessions[0]
    for l in range(1, k + 1):                                                      # :483
        kx = sessions[l - 1].reply(v)
        if tamper_reply is not None:
            kx = tamper_reply(l, kx)
        _write(dfr_file(nizkp, l), _reply_tree(grp, kx, keywidth))
        if l != 1:
            ver.setCommitment(l, *commitments[l])
            ver.setReply(l, kx)
    ver.combine(correct, y, comb)                                                  # :492-498
    ver.batchCombined()
    if not ver.verifyCombined(v):                                                  # :512-528: every party on its own
        for l in range(1, k + 1):
            ver.batch(l)
            correct[l] = ver.verify(l, v)
        for a in comb:
            a.free()
        comb = native.combineDecryptionFactors(F, correct, k, threshold, grp.q)
    plain = native.plaintexts(V, comb)                                             # :536-538
    _write(plaintexts_file(nizkp), _wide_array_tree(plain, keywidth))
    _write(cr_file(nizkp), _booleans_tree(correct))                                # :542
    for s in sessions:
        s.free()
    for a in comb + [c for fl in F[1:] for c in fl]:
        a.free()
    return plain


def verify_decryption(nizkp: str, grp, params: dict, pkey: Sequence, list_file: str, vectors: Optional[Dict[str, str]] = None,
                      keywidth: int = 1) -> bool:
    """The verifier's decryption branch (MixNetElGamalVerifyFiatShamirSession.java:1545-1667) for the list in `list_file`:
    read the correct indices (at least `threshold` of them, :1163-1174) and every party's factors, combine the indicated ones,
    derive the seed and the challenge, check the COMBINED proof, and match Plaintexts.bt with second components x combined
    factors.  k and the threshold are params["k"], params["threshold"].  `vectors` receives Dec.s (hexadecimal), Dec.v
    (decimal: integerChallenge.toString()) and the public key shares Dec.y_l = poly(l).  A missing file, a file that cannot be
    parsed or too few correct indices give False."""
    tv = vectors if vectors is not None else {}
    list_bytes = _read_file(list_file)
    if list_bytes is None or not os.path.exists(poly_file(nizkp)) or not os.path.exists(cr_file(nizkp)):
        return False
    W = parse_ciphertexts(grp, list_bytes, len(pkey) // 2 // keywidth, 0, keywidth)
    if W is None:
        return False
    ok, _ = dec_core(nizkp, grp, params, pkey, W, list_bytes, tv, keywidth)
    for a in W:
        a.free()
    return ok


def dec_core(nizkp: str, grp, params: dict, pkey: Sequence, W: Sequence[PGroupElementArray], list_bytes, tv: dict, keywidth: int = 1):
    """The decryption branch on a loaded list: its 2 omega component arrays W and the bytes of its tree (what the seed is
    hashed over).  Returns (verdict, the correct indices read from CorrectIndices.bt or None); frees nothing it was given."""
    D = _Derived.of(params)
    k, threshold = int(params["k"]), int(params["threshold"])
    width = len(pkey) // 2                                                         # components in all, kappa * omega
    n, omega = W[0].size(), width // keywidth
    keyed = {} if keywidth == 1 else {"keywidth": keywidth}
    poly_bt = _read_file(poly_file(nizkp))
    correct = _read_booleans(cr_file(nizkp), k + 1) if poly_bt is not None else None
    if correct is None or sum(1 for l in range(1, k + 1) if correct[l]) < threshold:
        return False, correct
    basic, made = None, []                                                         # the engine and the device arrays created here
    try:
        poly = parse_polynomial(grp, poly_bt, threshold, keywidth)
        if poly is None:
            return False, correct
        ys = [None] + [eval_keys(grp, poly, l, keywidth) for l in range(1, k + 1)]
        for l in range(1, k + 1):
            tv["Dec.y_%d" % l] = _hexk(ys[l], keywidth)
        F: List[Optional[List[PGroupElementArray]]] = [None]
        for l in range(1, k + 1):                                                  # getDecryptionFactors :1098-1114
            fl = _read_wide_array(grp, df_file(nizkp, l), omega, n, keywidth)
            if fl is None:
                return False, correct
            F.append(fl)
            made += fl
        U, V = W[:width], W[width:]
        try:
            comb = native.combineDecryptionFactors(F, correct, k, threshold, grp.q)     # :1569-1574
        except native.VmnError:
            return False, correct
        made += comb
        seed = _decryption_seed(D, grp, list_bytes, poly_bt, F[1:], keywidth)
        tv["Dec.s"] = seed.hex()                                                   # :1609
        basic = native.DistrElGamalSessionBasic(grp, 1, k, threshold, D.NE)
        basic.setInstance(U, ys, F, **keyed)
        basic.setBatchVectorSeed(seed)
        basic.batchInput()
        trees = []
        for l in range(1, k + 1):                                                  # readCommitments :1182-1190
            c = _read_commitment(grp, dfc_file(nizkp, l), omega, keywidth)
            if c is None:
                return False, correct
            try:
                basic.setCommitment(l, *c)
            except native.VmnError:
                return False, correct
            trees.append(_commitment_tree(grp, *c, keywidth))
        v = D.challenge(seed, fs._hdr(0, k) + b"".join(trees))
        tv["Dec.v"] = str(v)                                                       # :1634
        for l in range(1, k + 1):                                                  # readReplies :1198-1206
            buf = _read_file(dfr_file(nizkp, l))
            kx = _read_reply(grp, buf, keywidth) if buf is not None else None
            if kx is None:
                return False, correct
            basic.setReply(l, kx)
        try:
            basic.combine(correct, _y_rows(pkey, width, keywidth), comb)           # :1640-1644
            basic.batchCombined()
            verdict = basic.verifyCombined(v)
        except native.VmnError:
            return False, correct
        computed = native.plaintexts(V, comb)                                      # :1652-1663
        made += computed
        plain = _read_wide_array(grp, plaintexts_file(nizkp), omega, n, keywidth)
        made += plain or []
        return bool(verdict) and plain is not None and all(a.equals(b) for a, b in zip(plain, computed)), correct
    finally:
        if basic is not None:
            basic.free()
        for a in made:
            a.free()


# =============================================================================================================================
# The session: what `vmnv` verifies -- MixNetElGamalVerifyFiatShamirSession.verify (:1318-1670) over a whole directory
#     <nizkp>/version                  package version                           mixnet/MixNetElGamalSession.java:444
#     <nizkp>/type                     mixing | shuffling | decryption           :53-63, :423
#     <nizkp>/auxsid                   auxiliary session identifier              :381
#     <nizkp>/width                    width of the ciphertexts                  :434
#     <nizkp>/ShuffledCiphertexts.bt   output of a shuffling session             :403
#     <nizkp>/proofs/activethreshold   parties active in the shuffle             mixnet/ShufflerElGamalSession.java:1099
#     <nizkp>/proofs/maxciph           N_0; there iff precomputation was used    :1089, verifier :946
# The small files are written by VCR's ExtIO (unsafeWriteString / unsafeWriteInt), which is not part of the reference tree:
# [NOT-IN-REF].  Here: strings as UTF-8 text without a trailing newline, integers in decimal; surrounding whitespace is
# stripped on read.
# =============================================================================================================================
MIX_TYPE, SHUFFLE_TYPE, DECRYPT_TYPE = "mixing", "shuffling", "decryption"


class SessionFormatError(Exception):
    """The reference's failStop: the directory is not a session this verifier can check (a missing or inconsistent session
    file, a key that does not fit).  Not a verdict: a proof that does not verify gives a SessionVerdict, never this."""


def version_file(nizkp):
    return _p(nizkp, "version")


def type_file(nizkp):
    return _p(nizkp, "type")


def auxsid_file(nizkp):
    return _p(nizkp, "auxsid")


def width_file(nizkp):
    return _p(nizkp, "width")


def ls_file(nizkp):
    return _p(nizkp, "ShuffledCiphertexts.bt")


def at_file(nizkp):
    return _p(nizkp, "proofs", "activethreshold")


def mc_file(nizkp):
    return _p(nizkp, "proofs", "maxciph")


def write_string(path: str, value: str) -> None:
    """A small session file ([NOT-IN-REF]: ExtIO's own format is VCR code): UTF-8 text, no trailing newline."""
    _write(path, value.encode("utf-8"))


def write_int(path: str, value: int) -> None:
    write_string(path, "%d" % value)


def read_string(path: str) -> str:
    """The text of a small session file without surrounding whitespace.  Raises FileNotFoundError / OSError / UnicodeError."""
    with open(path, "rb") as f:
        return f.read().decode("utf-8").strip()


def _small(path: str, missing: str, unreadable: str) -> str:
    try:
        return read_string(path)
    except FileNotFoundError:
        raise SessionFormatError(missing) from None
    except (OSError, UnicodeError):
        raise SessionFormatError(unreadable) from None


def _small_int(path: str, missing: str, unreadable: str, unparsable: str) -> int:
    text = _small(path, missing, unreadable)
    if not re.fullmatch(r"[+-]?[0-9]+", text):              # Integer.parseInt
        raise SessionFormatError(unparsable)
    return int(text)


@dataclasses.dataclass(frozen=True)
class SessionParams:
    """mixnet/SessionParams.java: what the caller expects of a session (type None / auxsid None: take the proof's; width -1:
    take the proof's, 0: it must be the default width, > 0: it must be this) and which parts are verified."""
    type: Optional[str] = None
    auxsid: Optional[str] = None
    width: int = -1
    dec: bool = True
    posc: bool = True
    ccpos: bool = True


def verify_version(nizkp: str, params: dict, tv: dict) -> str:
    """verifyVersion (:295-318) against params["version"]."""
    version = _small(version_file(nizkp), "Can not find version file in proof directory!", "Can not read version from file!")
    if version != params["version"]:
        raise SessionFormatError("Expected package version %s but the proof was created by a package with version %s!"
                                 % (params["version"], version))
    tv["par.version"] = version
    return version


def determine_type(nizkp: str, expected: Optional[str]) -> str:
    """determineType (:327-358)."""
    actual = _small(type_file(nizkp), "Can not find type file in proof directory!", "Can not read type from type file!")
    if actual not in (MIX_TYPE, SHUFFLE_TYPE, DECRYPT_TYPE):
        raise SessionFormatError("Unknown type of proof! (%s)" % actual)
    if expected is not None and actual != expected:
        raise SessionFormatError("Attempting to verify proof of %s, but proof is a proof of %s!" % (expected, actual))
    return actual


def determine_auxsid(nizkp: str, expected: Optional[str]) -> str:
    """determineAuxsid (:369-396); Protocol.validateSid is VCR code ([NOT-IN-REF]): letters, digits and underscore."""
    actual = _small(auxsid_file(nizkp), "Can not find auxsid file in proof directory!", "Can not read auxsid from file!")
    if not re.fullmatch(r"[A-Za-z0-9_]+", actual):
        raise SessionFormatError("Invalid auxiliary session identifier in the proof! (%s)" % actual)
    if expected is not None and actual != expected:
        raise SessionFormatError("The given auxiliary session identifier does not match the one in the proof!")
    return actual


def determine_width(nizkp: str, expected: int, default: int, tv: dict) -> int:
    """determineWidth (:409-457): expected < 0 takes the proof's width, 0 matches it against the default, > 0 against itself."""
    actual = _small_int(width_file(nizkp), "Can not find width file in proof directory!", "Can not read width from file!",
                        "Can not parse width given in file!")
    if expected > 0:
        if actual != expected:
            raise SessionFormatError("The given width does not match the width in the proof!")
    elif expected == 0 and actual != default:
        raise SessionFormatError("The width in proof does not match the width in the protocol info file! Use the \"-width\" "
                                 "option to specify the width for which verification is performed.")
    if actual <= 0:
        raise SessionFormatError("Width is not positive!")
    tv["par.omega"] = str(actual)
    return actual


def determine_active_threshold(nizkp: str, threshold: int, k: int, tv: dict) -> int:
    """determineActiveThreshold (:465-501).  The reference prints it under the name par.lambda, which :1323 has already used for
    the threshold; here the threshold keeps par.lambda and the active threshold goes to vectors["par.lambda.active"]."""
    active = _small_int(at_file(nizkp), "Can not find active threshold file in proof directory!",
                        "Can not read active threshold from file!", "Can not parse active threshold given in file!")
    if active > k:
        raise SessionFormatError("Active threshold is larger than the number of mix-servers!")
    if active < threshold:
        raise SessionFormatError("Active threshold is smaller than threshold!")
    tv["par.lambda.active"] = str(active)
    return active


def read_maxciph(nizkp: str, tv: dict) -> int:
    """readMaxciph (:509-530)."""
    n0 = _small_int(mc_file(nizkp), "Can not find maxciph file in proof directory!", "Can not read from maxciph file!",
                    "Can not parse maxciph file!")
    tv["par.N_0"] = str(n0)
    return n0


def determine_session_params(nizkp: str, params: dict, expected: SessionParams, tv: dict) -> SessionParams:
    """determineSessionParams (:984-1006): a shuffling session has no decryption, a decryption session no shuffle; the width is
    only looked at when ciphertexts are."""
    typ = determine_type(nizkp, expected.type)
    auxsid = determine_auxsid(nizkp, expected.auxsid)
    width, dec, posc, ccpos = expected.width, expected.dec, expected.posc, expected.ccpos
    if typ == SHUFFLE_TYPE:
        dec = False
    elif typ == DECRYPT_TYPE:
        posc = ccpos = False
    if ccpos or dec:
        width = determine_width(nizkp, expected.width, int(params.get("width", 1)), tv)
    return SessionParams(typ, auxsid, width, dec, posc, ccpos)


@dataclasses.dataclass
class PartyVerdict:
    """One active party of the shuffle: its verdict as the loop (:1397-1518) computes it and the proofs behind it (None: not
    part of this flow or not looked at)."""
    l: int
    verdict: bool = True
    posc: Optional[bool] = None
    ccpos: Optional[bool] = None
    pos: Optional[bool] = None
    replaced: bool = False


@dataclasses.dataclass
class SessionVerdict:
    """What verify_session found.  `params`: the determined SessionParams; `parties`: one PartyVerdict per ACTIVE party, in
    order; `replaced`: the parties whose output was replaced by their input; `valid_proofs`: validProofs of :1394-1512;
    `decryption` / `correct`: the decryption's verdict and the correct indices it read (None when not verified).
    `accepted` is THIS LIBRARY's summary, not a value of the reference (which prints "Too few proofs are valid" as information
    and goes on, :1531-1534): enough valid proofs where shuffles were verified, and a valid decryption where it was."""
    params: SessionParams
    active_threshold: int
    precomp: bool
    parties: List[PartyVerdict]
    replaced: frozenset
    valid_proofs: int
    decryption: Optional[bool]
    correct: Optional[List[bool]]
    accepted: bool

    @property
    def verdicts(self) -> List[bool]:
        return [p.verdict for p in self.parties]


@dataclasses.dataclass
class SessionEngines:
    """The proof engines run_session drives.  Every one takes the session context `ctx` (nizkp, grp, params with the proof's
    auxsid, pkey = the widened key, keywidth = kappa) first; device arrays are opaque to the control flow.  With kappa > 1 g',
    y and a coefficient are kappa-tuples and a list has 2 kappa width arrays.
        read_pkey(ctx, path) -> [g', y] | None                 read_poly(ctx, path, threshold) -> coefficients | None
        read_list(ctx, path, data, width, n) -> list | None     (n = 0: any size)      list_size(ctx, list) -> N
        derive_generators(ctx, rho, n) -> (H, bytes of H's tree)                        copy_range(ctx, array, n) -> array
        read_commitment(ctx, data, n) -> U | None               shrink(ctx, l, U, n_max, n) -> U_s | None
        verify_posc(ctx, l, H, U, n_max, seed, tv) -> bool      verify_ccpos(ctx, l, H_s, U_s, W, WP, seed, tv) -> bool
        verify_pos(ctx, l, H, U, W, WP, seed, tv, with_arrays) -> bool
        verify_dec(ctx, W, data, tv) -> (bool, correct indices | None)
        hash_seed(ctx, kind, l, parts) -> seed bytes            (kind: "PoS" | "PoSC" | "CCPoS"; runs on worker threads)
        show(ctx, array) -> text                                free(ctx, arrays) -> None
    `seed` is a function without arguments: the engine calls it where the reference derives the seed."""
    read_pkey: Callable
    read_poly: Callable
    read_list: Callable
    list_size: Callable
    derive_generators: Callable
    copy_range: Callable
    read_commitment: Callable
    shrink: Callable
    verify_posc: Callable
    verify_ccpos: Callable
    verify_pos: Callable
    verify_dec: Callable
    hash_seed: Callable
    show: Callable
    free: Callable


# ---- the engines on the GPU ---------------------------------------------------------------------------------------------------
def _gpu_read_pkey(ctx, path):
    """An element of getCiphPGroup(plainPGroup, 1): node(g', y), each half node(kappa element trees) when kappa > 1."""
    got = _read_element_nests(ctx.grp, _read_file(path), (1, 1), ctx.keywidth)
    return [_unrows(rows, ctx.keywidth) for rows in got] if got is not None else None


def _gpu_read_poly(ctx, path, threshold):
    return parse_polynomial(ctx.grp, _read_file(path), threshold, ctx.keywidth)


def _gpu_derive_generators(ctx, rho, n):
    H = derive_generators(ctx.grp, ctx.params, rho, n)
    return H, H.toByteTree()


def _gpu_shrink(ctx, l, U, n_max, n):
    keep = read_keep_list(ctx.nizkp, l, n_max, n)
    return U.extract(keep) if keep is not None else None


def _gpu_free(ctx, arrays):
    for a in arrays:
        a.free()


GPU_ENGINES = SessionEngines(
    read_pkey=_gpu_read_pkey, read_poly=_gpu_read_poly,
    read_list=lambda ctx, path, data, width, n: parse_ciphertexts(ctx.grp, data, width, n, ctx.keywidth),
    list_size=lambda ctx, comps: comps[0].size(),
    derive_generators=_gpu_derive_generators,
    copy_range=lambda ctx, a, n: a.copyOfRange(0, n),
    read_commitment=lambda ctx, data, n: parse_commitment(ctx.grp, data, n),
    shrink=_gpu_shrink,
    verify_posc=lambda ctx, l, H, U, n_max, seed, tv: posc_core(ctx.nizkp, l, ctx.grp, ctx.params, H, U, n_max, seed, tv),
    verify_ccpos=lambda ctx, l, H_s, U_s, W, WP, seed, tv: ccpos_core(ctx.nizkp, l, ctx.grp, ctx.params, ctx.pkey, H_s, U_s, W, WP, seed, tv, ctx.keywidth),
    verify_pos=lambda ctx, l, H, U, W, WP, seed, tv, with_arrays: pos_core(ctx.nizkp, l, ctx.grp, ctx.params, ctx.pkey, W, WP, H, U, seed, tv, with_arrays, ctx.keywidth),
    verify_dec=lambda ctx, W, data, tv: dec_core(ctx.nizkp, ctx.grp, ctx.params, ctx.pkey, W, data, tv, ctx.keywidth),
    hash_seed=lambda ctx, kind, l, parts: _Derived.of(ctx.params).seed(parts),
    show=lambda ctx, a: "(" + ", ".join(_arr(c) for c in a) + ")" if isinstance(a, list) else _arr(a),
    free=_gpu_free)


# ---- files read once, seeds hashed ahead ------------------------------------------------------------------------------------------
class _Files:
    """The bytes of the directory's big files, each read once, for the protocol thread and the hashing threads alike."""

    def __init__(self):
        self._lock, self._data = threading.Lock(), {}

    def get(self, path: str) -> Optional[bytes]:
        with self._lock:
            if path not in self._data:
                self._data[path] = _read_file(path)
            return self._data[path]

    def drop(self, path: str) -> None:
        with self._lock:
            self._data.pop(path, None)


class _List:
    """One list file of the session: its bytes (what seeds are hashed over) and, once imported, its arrays.  The SAME object is
    the output of party l and the input of party l + 1, and the input object itself stands in for an output that is replaced."""

    def __init__(self, path: str, files: _Files):
        self.path, self.files, self.comps, self._tried = path, files, None, False

    def data(self) -> Optional[bytes]:
        return self.files.get(self.path)

    def load(self, ctx, eng, width: int, n: int):
        if not self._tried:
            self._tried = True
            data = self.data()
            self.comps = eng.read_list(ctx, self.path, data, width, n) if data is not None else None
        return self.comps

    def release(self, ctx, eng) -> None:
        if self.comps is not None:
            eng.free(ctx, self.comps)
        self.comps = None
        self.files.drop(self.path)


HASH_THREADS = 4


class _SeedsAhead:
    """Seeds of later parties, hashed on worker threads (hashlib releases the GIL) while the GPU verifies the party before them.
    A seed depends on files alone, except that the input of party l + 1 is party l's input when party l fails: every job records
    what it assumed, and `take` throws the job's result away unless that is what the party is verified with."""

    def __init__(self, enabled: bool, stats: Optional[dict]):
        self.pool = ThreadPoolExecutor(max_workers=HASH_THREADS) if enabled else None
        self.jobs, self.stats = {}, stats if stats is not None else {}
        self.stats.setdefault("ahead", [])
        self.stats.setdefault("used", [])
        self.stats.setdefault("discarded", [])

    def submit(self, key, assumed: tuple, job: Callable) -> None:
        if self.pool is not None and key not in self.jobs:
            self.stats["ahead"].append(key)
            self.jobs[key] = (assumed, self.pool.submit(job))

    def take(self, key, actual: tuple, job: Callable) -> bytes:
        got = self.jobs.pop(key, None)
        if got is not None:
            assumed, fut = got
            if len(assumed) == len(actual) and all(a is b for a, b in zip(assumed, actual)):
                seed = fut.result()
                if seed is not None:
                    self.stats["used"].append(key)
                    return seed
            else:
                fut.cancel()
                self.stats["discarded"].append(key)
        return job()

    def close(self) -> None:
        if self.pool is not None:
            self.pool.shutdown(wait=True, cancel_futures=True)


def _tree_prefix(grp, bt: bytes, n: int) -> bytes:
    """toByteTree() of copyOfRange(0, n) of the array whose tree is bt."""
    size = grp.array_tree_size(1) - 5
    return fs._hdr(0, n) + bt[5:5 + n * size]


def _tree_extract(grp, bt: bytes, keep: Sequence[bool]) -> bytes:
    """toByteTree() of extract(keep) of the array whose tree is bt."""
    size = grp.array_tree_size(1) - 5
    return fs._hdr(0, sum(keep)) + b"".join(bt[5 + i * size:5 + (i + 1) * size] for i, kept in enumerate(keep) if kept)


_FROM_FILE, _FROM_GENERATORS = object(), object()


def run_session(nizkp: str, grp, params: dict, expected: SessionParams, eng: SessionEngines,
                vectors: Optional[dict] = None, with_arrays: bool = False, stats: Optional[dict] = None,
                keywidth: Optional[int] = None) -> SessionVerdict:
    """The control flow of MixNetElGamalVerifyFiatShamirSession.verify (:1318-1670) over the engines `eng`: session files, keys,
    generators once, the chain of parties with its replacement rules, the decryption of the list the chain ends in.  See
    verify_session.  `stats` (a dict) receives which seeds were hashed ahead, used and discarded.  `keywidth`: the width of the
    public key; None takes params["keywidth"], 1 when params has none."""
    tv = vectors if vectors is not None else {}
    kw = int(params.get("keywidth", 1)) if keywidth is None else int(keywidth)
    if kw < 1:
        raise SessionFormatError("Key width is not positive!")
    k, threshold = int(params["k"]), int(params["threshold"])
    tv["par.k"], tv["par.lambda"] = str(k), str(threshold)                         # :1322-1331
    tv["par.n_e"], tv["par.n_r"], tv["par.n_v"] = str(int(params["ebitlenro"])), str(int(params["rbitlen"])), str(int(params["vbitlenro"]))
    tv["par.s_PRG"], tv["par.s_Gq"], tv["par.s_H"] = params["prg"], params["pgroup"], params["rohash"]
    verify_version(nizkp, params, tv)                                              # :1335
    sp = determine_session_params(nizkp, params, expected, tv)                     # :1338
    params = dict(params, auxsid=sp.auxsid)
    width = sp.width
    ctx = SimpleNamespace(nizkp=nizkp, grp=grp, params=params, pkey=None, keywidth=kw)
    # ---- readFullPKey :194-234
    if not os.path.exists(pk_file(nizkp)):
        raise SessionFormatError("Joint public key file %s can not be found!" % pk_file(nizkp))
    pk = eng.read_pkey(ctx, pk_file(nizkp))
    if pk is None:
        raise SessionFormatError("Could not read full El Gamal public key from file! (%s)" % pk_file(nizkp))
    tv["bas.pk"] = "(" + _hexk(pk[0], kw) + ", " + _hexk(pk[1], kw) + ")"
    if pk[0] != (grp.g if kw == 1 else (grp.g,) * kw):                             # plainPGroup.getg() :229
        raise SessionFormatError("Basic public key is not the standard generator!")
    if width > 0:
        ctx.pkey = list(_rows(pk[0], kw)) * width + list(_rows(pk[1], kw)) * width     # ProtocolElGamal.getWidePublicKey
    # ---- readMixServerPKeys :239-287
    if sp.dec:
        poly = eng.read_poly(ctx, poly_file(nizkp), threshold)
        if poly is None:
            raise SessionFormatError("Unable to read polynomial in exponent from file! (%s)" % poly_file(nizkp))
        ys = [None] + [eval_keys(grp, poly, l, kw) for l in range(1, k + 1)]
        if pk[1] != poly[0]:
            raise SessionFormatError("Mismatching public keys!")
        tv["bas.y_l"] = "(" + ",".join(_hexk(ys[l], kw) for l in range(1, threshold + 1)) + ")"
    # ---- the global prefix :158-189, :1351
    tv["par.sid"] = params["sid"]
    rho = global_prefix(params)
    tv["der.rho"] = rho.hex()
    precomp = os.path.exists(mc_file(nizkp))                                       # :946
    active = determine_active_threshold(nizkp, threshold, k, tv)                   # :1357
    files = _Files()
    # ---- readCiphertexts :1017-1046
    first = None
    if sp.ccpos or sp.dec:
        original = sp.ccpos or sp.type == DECRYPT_TYPE
        # otherwise the decryption alone of a directory that was mixed: start from the end of the shuffling
        path = l_file(nizkp, 0 if original else active)
        if original and not os.path.exists(path):
            raise SessionFormatError("Can not find array file! (%s)" % path)
        if os.path.exists(path):
            first = _List(path, files)
            if first.load(ctx, eng, width, 0) is None:
                raise SessionFormatError("Unable to read array %s!" % os.path.basename(path))
            if with_arrays:
                tv["bas.L_0"] = eng.show(ctx, first.comps)
    parties: List[PartyVerdict] = []
    replaced = set()
    valid = 0
    inp = first
    if sp.posc or sp.ccpos:
        if precomp:
            maxciph = read_maxciph(nizkp, tv)                                      # getMaxciph :541-548
        elif first is None:
            raise SessionFormatError("No ciphertexts to take the number of generators from!")   # (the reference dereferences null)
        else:
            maxciph = eng.list_size(ctx, first.comps)
        n = eng.list_size(ctx, first.comps) if first is not None else 0
        if n > maxciph:
            raise SessionFormatError("Too few generators have been derived!")      # :572-574
        H, H_bt = eng.derive_generators(ctx, rho, maxciph)                         # deriveGenerators :556-576, once
        if with_arrays:
            tv["bas.h"] = eng.show(ctx, H)
        H_s = eng.copy_range(ctx, H, n) if sp.ccpos and precomp else None          # getShrunkGenerators :1059-1068
        env = os.environ.get("VMN_SESSION_HASH_AHEAD", "1")
        ahead = _SeedsAhead(env != "0", stats)
        g_tree = grp.element_tree(grp.g)
        pk_tree = fs.product_element_tree(grp, ctx.pkey, kw) if ctx.pkey else None
        posc_active = lambda l: os.path.exists(pc_file(nizkp, l))                  # :958-962
        ccpos_active = lambda l: os.path.exists(ccposc_file(nizkp, l)) or os.path.exists(posc_file(nizkp, l))      # :972-976
        is_active = lambda l: (sp.posc and precomp and not sp.ccpos and posc_active(l)) or ccpos_active(l)

        def out_list(l):
            path = l_file(nizkp, l)
            if l == active and not os.path.exists(path):                           # :1446-1449
                path = ls_file(nizkp)
            return _List(path, files)
        outs = {l: out_list(l) for l in range(1, active + 1)} if sp.ccpos else {}

        def commitment_bytes(l, source):
            return files.get(pc_file(nizkp, l)) if source is _FROM_FILE else H_bt

        def posc_job(l):
            def job():
                u_bt = files.get(pc_file(nizkp, l))
                return eng.hash_seed(ctx, "PoSC", l, posc_seed_parts(g_tree, H_bt, u_bt)) if u_bt is not None else None
            return job

        def shuffle_job(l, src, dst, source):
            """The seed of party l's PoS / CCPoS over the lists src -> dst and the commitment read from `source`."""
            def job():
                u_bt, a, b = commitment_bytes(l, source), src.data(), dst.data()
                if u_bt is None or a is None or b is None:
                    return None
                if not precomp:
                    return eng.hash_seed(ctx, "PoS", l, shuffle_seed_parts(g_tree, H_bt, u_bt, pk_tree, a, b))
                keep = read_keep_list(nizkp, l, maxciph, n)
                if keep is None:
                    return None
                return eng.hash_seed(ctx, "CCPoS", l, shuffle_seed_parts(g_tree, _tree_prefix(grp, H_bt, n), _tree_extract(grp, u_bt, keep),
                                                                         pk_tree, a, b))
            return job

        def hash_ahead(l, src):
            """Start on party l's seeds, assuming the party before it is valid (its input is then `src`)."""
            if l <= active and is_active(l):
                if sp.posc and precomp:
                    ahead.submit(("PoSC", l), (), posc_job(l))
                if sp.ccpos:
                    ahead.submit(("shuffle", l), (src, outs[l], _FROM_FILE), shuffle_job(l, src, outs[l], _FROM_FILE))
        try:
            hash_ahead(1, inp)
            for l in range(1, active + 1):                                         # :1397-1518
                verdict = True
                if is_active(l):
                    ptv = tv.setdefault("party", {}).setdefault(l, {})
                    pv = PartyVerdict(l)
                    source = _FROM_FILE
                    U = eng.read_commitment(ctx, files.get(pc_file(nizkp, l)), maxciph)      # readPermutationCommitment :626-641
                    if with_arrays and U is not None:
                        ptv["u"] = eng.show(ctx, U)
                    hash_ahead(l + 1, outs.get(l))
                    if sp.posc and precomp:                                        # :1416-1437
                        pv.posc = U is not None and bool(eng.verify_posc(ctx, l, H, U, maxciph,
                                                                         lambda: ahead.take(("PoSC", l), (), posc_job(l)), ptv))
                        if not pv.posc:
                            verdict = False
                            if U is not None:
                                eng.free(ctx, [U])
                            U, source = eng.copy_range(ctx, H, maxciph), _FROM_GENERATORS
                    if sp.ccpos:
                        out = outs[l]
                        WP = out.load(ctx, eng, width, n)                          # :1446-1451
                        if with_arrays and WP is not None:
                            ptv["bas.L_l"] = eng.show(ctx, WP)
                        seed = lambda: ahead.take(("shuffle", l), (inp, out, source), shuffle_job(l, inp, out, source))
                        if precomp:                                                # :1457-1477
                            U_s = eng.shrink(ctx, l, U, maxciph, n) if U is not None and WP is not None else None
                            pv.ccpos = U_s is not None and bool(eng.verify_ccpos(ctx, l, H_s, U_s, inp.comps, WP, seed, ptv))
                            verdict = verdict and pv.ccpos
                            if U_s is not None:
                                eng.free(ctx, [U_s])
                        else:                                                      # :1481-1487
                            pv.pos = U is not None and WP is not None and \
                                bool(eng.verify_pos(ctx, l, H, U, inp.comps, WP, seed, ptv, with_arrays))
                            verdict = pv.pos
                        if verdict:
                            inp.release(ctx, eng)
                            inp = out
                        else:                                                      # :1494-1502: the input itself, not a re-read
                            out.release(ctx, eng)
                            pv.replaced = True
                            replaced.add(l)
                    if U is not None:
                        eng.free(ctx, [U])
                    if verdict:
                        valid += 1
                    pv.verdict = verdict
                    parties.append(pv)
        finally:
            ahead.close()
        eng.free(ctx, [H] + ([H_s] if H_s is not None else []))
    accepted = not (sp.posc or sp.ccpos) or valid >= threshold                     # :1531-1534 prints and goes on
    dec_verdict = correct = None
    if sp.dec:                                                                     # :1537-1667
        if inp is None:
            raise SessionFormatError("Can not find array file! (%s)" % l_file(nizkp, active))
        dec_verdict, correct = eng.verify_dec(ctx, inp.comps, inp.data(), tv)
        dec_verdict = bool(dec_verdict)
        accepted = accepted and dec_verdict
    if inp is not None:
        inp.release(ctx, eng)
    return SessionVerdict(sp, active, precomp, parties, frozenset(replaced), valid, dec_verdict, correct, accepted)


def verify_session(nizkp: str, grp, params: dict, expected: SessionParams = SessionParams(), vectors: Optional[dict] = None,
                   with_arrays: bool = False, keywidth: Optional[int] = None) -> SessionVerdict:
    """What `vmnv` does with a proof directory (MixNetElGamalVerifyFiatShamirSession.verify :1318-1670), on the GPU:
    the session files (version, type, auxsid, width, proofs/activethreshold, proofs/maxciph), the keys (FullPublicKey.bt =
    (g, y) at width 1, widened here; with a decryption the polynomial in the exponent, whose element 0 is y), the generators
    derived ONCE for maxciph, the chain L_0 -> L_1 -> ... of the active parties -- a failed PoSC sets the commitment to the
    generators and costs the verdict, a failed shuffle replaces the party's output by its input, the last output falls back to
    ShuffledCiphertexts.bt -- the count of valid proofs, the decryption of the list the chain ends in, Plaintexts.bt.

    A violated session check (the reference's failStop) raises SessionFormatError.  A per-party file that is missing or cannot
    be parsed (commitment, list, keep list, proof message) FAILS THAT PARTY, as verify_shuffle / verify_precomputed_shuffle do;
    the reference stops at some of these (readArray :588-616).  k, threshold, version, the default width and what goes into
    der.rho come from `params` (params.json); the auxsid is the proof's.

    Every list file is read and imported once; the generators' tree is exported once; the seeds of party l + 1 are hashed on up
    to HASH_THREADS worker threads while party l is verified (VMN_SESSION_HASH_AHEAD=0, read per call, turns that off: same
    verdicts, same vectors).  Two parts of the reference's output are not produced: bas.C_omega / bas.R_omega / bas.M_omega
    (VCR's toString() of groups, [NOT-IN-REF]).

    `vectors` receives, in the reference's names: par.k, par.lambda (the threshold), par.lambda.active (the active threshold,
    which the reference prints under par.lambda a second time, :498), par.n_e, par.n_r, par.n_v, par.s_PRG, par.s_Gq, par.s_H,
    par.version, par.omega, par.N_0, par.sid, bas.pk, bas.y_l, der.rho, Dec.*; with `with_arrays` bas.h and bas.L_0; and
    vectors["party"][l] = the PoS.* / PoSC.* / CCPoS.* vectors of party l (with `with_arrays` also u and bas.L_l).

    Under a public key of width kappa (`keywidth`, by default params["keywidth"], 1 when absent) FullPublicKey.bt is an element
    of getCiphPGroup(G^kappa, 1) whose first half must be (g, .., g) (:205-231), the coefficients of the polynomial lie in
    G^kappa, the lists have 2 kappa width arrays, and bas.pk, bas.y_l, Dec.y_l show an element of G^kappa as the tuple of its
    rows; the files are nested as the head of this module says."""
    return run_session(nizkp, grp, params, expected, GPU_ENGINES, vectors, with_arrays, keywidth=keywidth)


# ---- the writer: all k parties of a session -----------------------------------------------------------------------------------------
def write_session(nizkp: str, grp, params: dict, session_type: str, W: Sequence, y, rand, k: int, threshold: int,
                  active: Optional[int] = None, n0: int = 0, failing=(), poly: Optional[Sequence] = None,
                  shares: Optional[Sequence] = None, writers=None, keywidth: int = 1):
    """Every party of a session of `session_type` (mixing / shuffling / decryption) on the list W (2 * width component arrays)
    under the key (g, y), y = poly[0]: write_inputs, then for the active parties l = 1 .. `active` (default: threshold)
    write_shuffle, or with n0 > 0 write_precomputation for N_0 = n0 and write_committed_shuffle, then write_decryption with `poly`
    and `shares` (as write_decryption takes them).  Returns (params as written to params.json, the plaintexts or None).

    Files as the reference places them: version, auxsid, width (MixNetElGamalSession.java:219-223, 287-290),
    proofs/activethreshold and proofs/maxciph (ShufflerElGamalSession.java:394, 520, 593); proofs/Ciphertexts%02d.bt for
    l <= active in the plain flow (:225-235) and for l < active in the committed flow (:821, :953); ShuffledCiphertexts.bt and
    type = shuffling (MixNetElGamalSession.java:236-243); a mixing session renames ShuffledCiphertexts.bt into proofs/ and sets
    type = mixing (:294-303); a decryption-only session has Ciphertexts.bt and type = decryption (:305-310).  FullPublicKey.bt
    is (g, y) at width 1 (readFullPKey :205-212).  Two places where this writer does not follow the letter of the reference:
    the renamed list goes to proofs/Ciphertexts<active>.bt -- the reference names it by its `threshold` field, which is the same
    file when active = threshold and would otherwise overwrite the output of party `threshold`, while the verifier looks for
    the last list under the ACTIVE threshold (:1035, :1446); and a decryption-only session also gets proofs/activethreshold,
    which the verifier reads for every type (:1357).

    `failing`: parties that publish an invalid proof -- the party's honest commitment with the reply of a second, unrelated run
    on the same input.  The honest parties then go on as ShufflerElGamalSession.java:317-329: the party's output is replaced by
    its input (also in the file they keep for the verifier) and the next party shuffles that.

    `keywidth` = kappa > 1: W has 2 kappa width arrays, `y`, every coefficient of `poly` (a polynomial over Z_q^kappa in the
    exponent, y = poly[0]) and every share are kappa-tuples; FullPublicKey.bt is (g, .., g, y_0, .., y_(kappa-1)), the width file
    holds omega, params.json gains "keywidth" and every writer is handed keywidth=kappa.  With kappa = 1 nothing is handed on and
    params.json has no such entry: the directory is byte for byte the one written without the parameter."""
    wr = writers if writers is not None else SimpleNamespace(
        write_inputs=write_inputs, write_shuffle=write_shuffle, write_precomputation=write_precomputation,
        write_committed_shuffle=write_committed_shuffle, write_decryption=write_decryption)
    if session_type not in (MIX_TYPE, SHUFFLE_TYPE, DECRYPT_TYPE):
        raise ValueError("unknown session type %r" % (session_type,))
    active = threshold if active is None else active
    if not threshold <= active <= k:
        raise ValueError("threshold <= active <= k")
    if keywidth < 1 or len(W) % (2 * keywidth):
        raise ValueError("a list under a key of width kappa has 2 * kappa * width component arrays")
    width = len(W) // 2 // keywidth
    params = dict(params, k=k, threshold=threshold, width=width, N_0=n0)
    keyed = {}
    if keywidth > 1:
        params["keywidth"] = keywidth
        keyed["keywidth"] = keywidth
    g = grp.g
    wide = [g] * (keywidth * width) + list(_rows(y, keywidth)) * width
    os.makedirs(_p(nizkp, "proofs"), exist_ok=True)
    wr.write_inputs(nizkp, grp, params, [g] * keywidth + list(_rows(y, keywidth)), W, **keyed)
    write_string(version_file(nizkp), params["version"])
    write_string(auxsid_file(nizkp), params["auxsid"])
    write_int(width_file(nizkp), width)
    write_int(at_file(nizkp), active)
    last = list(W)
    if session_type != DECRYPT_TYPE:
        if n0:
            write_int(mc_file(nizkp), n0)
        pre, H = {}, None
        for l in range(1, active + 1) if n0 else ():
            pre[l] = wr.write_precomputation(nizkp, l, grp, params, n0, rand, H, **keyed)
            H = pre[l][3]

        def play(where, l, inp, out_file, secrets):
            if n0:
                return wr.write_committed_shuffle(where, l, grp, params, wide, inp, rand, *secrets, out_file=out_file, **keyed)
            return wr.write_shuffle(where, l, grp, params, wide, inp, rand, out_file=out_file, **keyed)
        for l in range(1, active + 1):
            out_file = ls_file(nizkp) if n0 and l == active else l_file(nizkp, l)
            out = play(nizkp, l, last, out_file, pre.get(l))
            if l in failing:
                with tempfile.TemporaryDirectory(dir=nizkp) as other:
                    os.makedirs(_p(other, "proofs"))
                    shutil.copyfile(l_file(nizkp, l - 1), l_file(other, l - 1))
                    secrets = wr.write_precomputation(other, l, grp, params, n0, rand, H, **keyed) if n0 else None
                    play(other, l, last, l_file(other, l), secrets)
                    reply = ccposr_file if n0 else posr_file
                    shutil.copyfile(reply(other, l), reply(nizkp, l))
                shutil.copyfile(l_file(nizkp, l - 1), out_file)
            else:
                last = out
        if not n0:
            shutil.copyfile(l_file(nizkp, active), ls_file(nizkp))
        write_string(type_file(nizkp), SHUFFLE_TYPE)
    plain = None
    if session_type != SHUFFLE_TYPE:
        if os.path.exists(ls_file(nizkp)):
            write_string(type_file(nizkp), MIX_TYPE)
            os.replace(ls_file(nizkp), l_file(nizkp, active))
        else:
            write_string(type_file(nizkp), DECRYPT_TYPE)
        plain = wr.write_decryption(nizkp, grp, params, wide, last, poly, shares, rand, k, threshold, **keyed)
    return params, plain
