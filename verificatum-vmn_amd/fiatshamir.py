"""fiatshamir.py — the Fiat-Shamir hashing around a proof, overlapped with the GPU work that does not depend on it.

Mirrors
  * ``ChallengerRO.challenge`` — RO_nout(globalPrefix || bytetree(data)),
    ref: src/java/com/verificatum/protocol/hvzk/ChallengerRO.java:96-116;
  * the two challenges of ``PoSTW`` / ``PoSCTW`` / ``CCPoSW``: the seed of the batching vector
    = challenge(node(g, h, u, pkey, w, w'), 8 * prg.minNoSeedBytes()) and the challenge
    v = challenge(node(leaf(seed), commitment), vbitlen), ref: hvzk/PoSTW.java:118-130, 146-151 (prover), 215-229,
    248-254 (verifier); hvzk/CCPoSW.java:75-158.

The digest is ONE sequential SHA-2 stream over all the byte trees (1.57 GB for the instance of a width-1 shuffle of
10^6 ciphertexts over a 2048-bit group: ~0.75 s on one host core), so it cannot be made faster -- only hidden: the
``InstanceHasher`` thread is the party's helper thread (``Context.helper()``, ``vmn_ctx_helper_begin``); it frames each
array on the GPU on the helper lane's own stream, downloads it into a page-locked buffer and feeds it to hashlib
(which releases the GIL), while the protocol thread keeps the GPU busy with the work that does not need the seed
(re-encryption, the permutation commitment, ``commitPrepare()``).
"""
from __future__ import annotations

import hashlib
import queue
import threading
from typing import Optional, Sequence


def _hdr(tag: int, n: int) -> bytes:
    return bytes([tag]) + int(n).to_bytes(4, "big")


def leaf(data: bytes) -> bytes:
    return _hdr(1, len(data)) + bytes(data)


def prg_bytes(seed: bytes, nbytes: int, hashname: str = "sha256") -> bytes:
    """PRGHeuristic: H(seed || uint32_be(0)) || H(seed || uint32_be(1)) || ..."""
    out = bytearray()
    ctr = 0
    while len(out) < nbytes:
        out += hashlib.new(hashname, seed + ctr.to_bytes(4, "big")).digest()
        ctr += 1
    return bytes(out[:nbytes])


class Challenger:
    """``ChallengerRO``: a random oracle with a global prefix (ProtocolElGamal.java:659-683 builds the prefix)."""

    def __init__(self, globalPrefix: bytes, hashname: str = "sha256"):
        self.prefix, self.hashname = bytes(globalPrefix), hashname

    def start(self, nout_bits: int):
        """The running digest of RandomOracle(H, nout).getDigest() after update(globalPrefix)."""
        return hashlib.new(self.hashname, int(nout_bits).to_bytes(4, "big") + self.prefix)

    def finish(self, digest, nout_bits: int) -> bytes:
        nb = (nout_bits + 7) // 8
        out = bytearray(prg_bytes(digest.digest(), nb, self.hashname))
        if nout_bits % 8:
            out[0] &= (1 << (nout_bits % 8)) - 1
        return bytes(out)

    def challenge(self, data: bytes, nout_bits: int) -> bytes:
        d = self.start(nout_bits)
        d.update(data)
        return self.finish(d, nout_bits)


def element_tree(group, els: Sequence) -> bytes:
    """Byte tree of a (product-)group element given as its 2*width components [a_1..a_w, b_1..b_w] (a wide key, a
    ciphertext-shaped commitment): node(leaf, leaf) at width 1, node(node(w leaves), node(w leaves)) otherwise; one
    element alone is a leaf."""
    enc = [leaf(group.enc_el(e)) for e in els]
    if len(enc) == 1:
        return enc[0]
    if len(enc) == 2:
        return _hdr(0, 2) + enc[0] + enc[1]
    half = len(enc) // 2
    return _hdr(0, 2) + _hdr(0, half) + b"".join(enc[:half]) + _hdr(0, half) + b"".join(enc[half:])


def group_element_tree(enc: bytes, cw: Optional[int] = None) -> bytes:
    """Byte tree of ONE group element given as its fixed-width encoding (``group.enc_el``).  ``cw`` = None: an element of a
    modular group, a leaf.  ``cw`` = the coordinate width of a curve group (``ECqPGroup.nbytes``): enc = x || y and the tree is
    node(leaf(x), leaf(y)) -- what the C++ message container and the array export write for a point; the point at infinity
    (enc = 2 cw bytes 0xff) comes out as two leaves of 0xff bytes, (-1, -1)."""
    if cw is None:
        return leaf(enc)
    if len(enc) != 2 * cw:
        raise ValueError("a point is two coordinates of %d bytes" % cw)
    return _hdr(0, 2) + leaf(enc[:cw]) + leaf(enc[cw:])


def array_tree_size(n: int, elem_bytes: int, cw: Optional[int] = None) -> int:
    """Bytes of the byte tree of an array of n group elements: node(n leaves of elem_bytes) over a modular group, node(n point
    nodes) = 5 + n (15 + 2 cw) over a curve with coordinate width cw (``vmn_garray_bytetree_size``)."""
    return 5 + n * (5 + elem_bytes if cw is None else 15 + 2 * cw)


def nested_tree(trees: Sequence[bytes], keywidth: int = 1) -> bytes:
    """The tree of an element (an array, a ring element) of (X^kappa)^omega given as the trees of its kappa * omega factors in
    flat order, factor l * kappa + j the key j of plaintext component l: [omega > 1: node(omega; ...)] over [kappa > 1:
    node(kappa; ...)] over the factors' own trees (a product is the node of its factors' trees; the plaintext
    group under a key of width kappa is G^kappa, MixNetElGamalVerifyFiatShamir.java:316-317).  kappa = 1: node(omega trees), the
    tree itself at omega = 1; omega = 1: node(kappa trees), the bytes of the unkeyed form of width kappa."""
    if keywidth < 1 or len(trees) % keywidth:
        raise ValueError("%d factors are no multiple of the key width %d" % (len(trees), keywidth))
    omega = len(trees) // keywidth
    inner = [b"".join(trees[l * keywidth:(l + 1) * keywidth]) for l in range(omega)]
    if keywidth > 1:
        inner = [_hdr(0, keywidth) + t for t in inner]
    return inner[0] if omega == 1 else _hdr(0, omega) + b"".join(inner)


class NoSuchTree(Exception):
    """The bytes under a ``Cursor`` are not the tree its caller asks for: a wrong tag, a wrong count, a short buffer, bytes
    behind the end.  Private to the readers: each catches it at its entry point and answers None."""


class Cursor:
    """A position in the bytes of a byte tree, moved by the one who knows which tree to expect: THE reader of the proof
    directory's framing (``_hdr``, ``leaf`` and ``nested_tree`` write it).  Every operation raises ``NoSuchTree`` -- never
    IndexError -- where the bytes are not what it was asked for."""

    def __init__(self, buf: bytes, pos: int = 0):
        self.buf, self.pos = buf, pos

    def _header(self, tag: int, move: bool = True) -> int:
        head = bytes(self.buf[self.pos:self.pos + 5])
        if len(head) != 5 or head[0] != tag:
            raise NoSuchTree()
        if move:
            self.pos += 5
        return int.from_bytes(head[1:], "big")

    def node(self, count: Optional[int] = None) -> int:
        """Step into a node (of ``count`` children, when given); its child count."""
        if count is not None and self._header(0, False) != count:
            raise NoSuchTree()
        return self._header(0)

    def children(self) -> int:
        """The child count of the node here, without stepping into it (an array tree says its own size)."""
        return self._header(0, False)

    def leaf(self, length: int) -> bytes:
        """The data of a leaf of ``length`` bytes."""
        if self._header(1, False) != length or len(self.buf) < self.pos + 5 + length:
            raise NoSuchTree()
        self.pos += 5
        return self.take(length)

    def take(self, size: int) -> bytes:
        """The next ``size`` bytes, a subtree whose size the caller knows, for the caller's own reader."""
        if size < 0 or len(self.buf) < self.pos + size:
            raise NoSuchTree()
        self.pos += size
        return self.buf[self.pos - size:self.pos]

    def item(self, read):
        """The value of ``read(buf, pos) -> (value, next position) | None`` (``group.element_from_tree``) here."""
        got = read(self.buf, self.pos)
        if got is None:
            raise NoSuchTree()
        self.pos = got[1]
        return got[0]

    def nested(self, width: int, keywidth: int, item) -> list:
        """The kappa * omega values of ``nested_tree``, each read by ``item(cursor)``, in flat order."""
        if width > 1:
            self.node(width)
        values = []
        for _ in range(width):
            if keywidth > 1:
                self.node(keywidth)
            values += [item(self) for _ in range(keywidth)]
        return values

    def end(self) -> None:
        """The tree fills its buffer."""
        if self.pos != len(self.buf):
            raise NoSuchTree()


def product_element_tree(group, els: Sequence, keywidth: int = 1) -> bytes:
    """``element_tree`` for any kind of group: the same shapes (one element alone: its own tree; node(a, b) at width 1;
    node(node(w trees), node(w trees)) otherwise) over the trees of the single elements, which are leaves for a modular group
    and point nodes for a curve (``group.coord_bytes``: the coordinate width, None / absent for a modular group).  Over a
    modular group the bytes are those of ``element_tree``.  ``keywidth`` = kappa > 1: each half is ``nested_tree`` of its
    kappa * omega element trees."""
    cw = getattr(group, "coord_bytes", None)
    enc = [group_element_tree(group.enc_el(e), cw) for e in els]
    if len(enc) == 1:
        return enc[0]
    half = len(enc) // 2
    return _hdr(0, 2) + nested_tree(enc[:half], keywidth) + nested_tree(enc[half:], keywidth)


def wide_element_tree(group, els: Sequence, keywidth: int = 1) -> bytes:
    """An element of G^omega given as its omega components: node(omega element trees), the element's own tree at omega = 1;
    with ``keywidth`` = kappa an element of (G^kappa)^omega given as its kappa * omega components (``nested_tree``)."""
    cw = getattr(group, "coord_bytes", None)
    return nested_tree([group_element_tree(group.enc_el(e), cw) for e in els], keywidth)


class InstanceHasher(threading.Thread):
    """Streams byte strings and the byte trees of device arrays into one digest, on the context's helper lane.

    Items are queued by the protocol thread in hashing order: ``put_bytes``, ``put_array``, ``put_ciphertexts`` (a
    ciphertext array = node(first components, second components)), ``mark()`` (the arrays queued from here on were
    produced by GPU work the protocol thread has queued up to now), ``finish()`` -> the digest object.
    """

    def __init__(self, ctx, digest, max_array_bytes: int):
        super().__init__(daemon=True)
        import torch
        self.ctx, self.digest = ctx, digest
        self.buf = torch.empty(max_array_bytes, dtype=torch.uint8).pin_memory()
        self.view = memoryview(self.buf.numpy())
        self.q: "queue.Queue" = queue.Queue()
        self.error: Optional[BaseException] = None
        self.bytes_hashed = 0
        self.busy_s = 0.0
        self.start()

    # ---- protocol thread ---------------------------------------------------------------------------------------
    def put_bytes(self, data: bytes):
        self.q.put(("bytes", bytes(data)))

    def put_array(self, arr):
        self.q.put(("array", arr))

    def put_ciphertexts(self, comps: Sequence):
        """A PPGroupElementArray of width w given as 2w component arrays: node(u-part, v-part), a part being the array's
        own tree at width 1 and node(w array trees) otherwise (component-array-wise)."""
        half = len(comps) // 2
        self.put_bytes(_hdr(0, 2))
        for part in (comps[:half], comps[half:]):
            if half > 1:
                self.put_bytes(_hdr(0, half))
            for a in part:
                self.put_array(a)

    def mark(self):
        self.ctx.helper_mark()
        self.q.put(("sync",))

    def finish(self):
        self.q.put(("end",))
        self.join()
        if self.error is not None:
            raise self.error
        return self.digest

    # ---- helper thread -----------------------------------------------------------------------------------------
    def run(self):
        import time
        try:
            with self.ctx.helper() as lane:
                while True:
                    item = self.q.get()
                    if item[0] == "end":
                        break
                    t0 = time.perf_counter()
                    if item[0] == "sync":
                        lane.sync()
                    elif item[0] == "bytes":
                        self.digest.update(item[1])
                        self.bytes_hashed += len(item[1])
                    else:
                        n = item[1].toByteTreeInto(self.buf)
                        self.digest.update(self.view[:n])
                        self.bytes_hashed += n
                    self.busy_s += time.perf_counter() - t0
        except BaseException as exc:      # pragma: no cover - re-raised by finish()
            self.error = exc
            while True:                    # drain, so that the protocol thread never blocks on a dead consumer
                try:
                    if self.q.get(timeout=0.1)[0] == "end":
                        break
                except queue.Empty:
                    break


def hash_instance(hasher: InstanceHasher, group, g, h, u, pkey, w, wp):
    """Queue node(g, h, u, pkey, w, w') in the reference's order (PoSTW.java:118-125).  u / wp may be None: the caller
    queues them later (after ``hasher.mark()``) with ``put_array`` / ``put_ciphertexts``."""
    hasher.put_bytes(_hdr(0, 6) + leaf(group.enc_el(g)))
    hasher.put_array(h)
    if u is not None:
        hasher.put_array(u)
        hasher.put_bytes(element_tree(group, pkey))
        hasher.put_ciphertexts(w)
        if wp is not None:
            hasher.put_ciphertexts(wp)
