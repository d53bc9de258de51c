"""interface.py — the files in front of a session: ciphertext lists, plaintexts and the public key in the reference's interfaces.

``raw``     one byte tree holding the 2w component arrays (``proofdir.read_ciphertexts`` / ``write_ciphertexts``): what
            the mix-net works on and what a proof directory holds.
``native``  the reference's default (``ProtocolElGamalInterfaceNative`` / ``...SeqHex``, ``CiphertextReaderLine``,
            ``CiphertextWriterLine``): one ciphertext per line, the line being the hexadecimal byte tree of that single
            ciphertext.  A ballot box delivers this; the first command of an election is ``vmnc -ciphs -ini native -outi raw``.

``json``    ``ProtocolElGamalInterfaceJSON`` / ``...JSONDecode``, the format of Helios-style ballot boxes, modular groups only:
            a ciphertext line is ``{"alpha":"A","beta":"B"}`` (an array of such pairs at width > 1), a plaintext line ``"M"``,
            the public key one map ``{"g":..,"p":..,"q":..,"y":..,"encoding":..}``; every number is a decimal string.

The native text is an array of structures, the arrays are a structure of arrays: the N lines are found, decoded, checked and
transposed on the GPU (``vmn_garrays_from_hexlines`` / ``vmn_garrays_to_hexlines``, csrc/light_kernels.h), not in a loop over
the lines; ``read_ciphertexts`` / ``write_ciphertexts`` / ``convert_ciphertexts`` are the file functions of these two interfaces.
The json text is converted from and to decimal on the GPU as well (``vmn_garrays_from_jsonlines`` / ``_to_jsonlines`` /
``_to_jsonplain``, csrc/decimal_kernels.h); ``read_list`` / ``write_list`` / ``convert_list`` take all three interfaces.  All readers
apply one policy to what enters here from outside: a format defect, a value out of range or an element outside the group is no
list (``None``).

Behind a session the plaintexts are text (``vmnc -plain -outi native``, ProtocolElGamalInterfaceString.decodePlaintexts): a
message of up to ``encode_length`` bytes per component is an element of a safe-prime group (csrc/encode_layout.h states the
encoding).  ``encode_texts`` / ``decode_texts`` convert whole lists on the GPU (``vmn_garrays_from_textlines`` /
``vmn_garrays_to_textlines``, csrc/encode_kernels.h), ``read_texts`` / ``write_decoded_plaintexts`` are their file functions, and
``demo_texts`` / ``demo_ciphertexts`` are the reference's dummy messages and their encryptions.  ``write_plaintexts`` and
``PLAINTEXT_FORMATS`` keep to ``json`` and ``raw``.  Over a curve group a message of up to ``point_encode_length`` bytes is the x
coordinate of a point under a one-byte counter (csrc/ec_encode_layout.h); ``encode_point_texts`` / ``decode_point_texts``,
``read_point_texts`` / ``write_decoded_point_plaintexts`` and ``demo_point_ciphertexts`` are the namesakes there
(``vmn_ec_arrays_from_textlines`` / ``vmn_ec_arrays_to_textlines``, csrc/ec_encode_kernels.h); the functions above keep refusing curves.

Under a public key of width kappa (``keywidth``, 1 by default) a ciphertext of ``width`` omega has 2 kappa omega components and
every half of a list or of a line one more node level (``proofdir``'s head, ``vmn_garrays_from_hexlines_keyed``); ``native`` and
``raw`` take it, ``json`` does not: the reference's JSON classes cast the components to elements of a modular group, so they
cannot hold such a list, and ``keywidth`` > 1 with ``json`` is a ``ValueError``.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import List, Optional, Sequence

from . import PGroupElementArray, _check, host_block, lib
from . import proofdir

FORMATS = ("native", "raw")                  # what read_ciphertexts / write_ciphertexts / convert_ciphertexts take
INTERFACES = FORMATS + ("json",)             # what read_list / write_list / convert_list take
PLAINTEXT_FORMATS = ("json", "raw")


def ciphertext_line_bytes(grp, width: int, keywidth: int = 1) -> int:
    """B: the bytes of one ciphertext of ``width`` over ``grp`` as a byte tree; a native line has 2B hex digits."""
    return lib().vmn_hexlines_line_bytes_keyed(grp._h, C.c_size_t(keywidth), C.c_size_t(width))


def _no_keyed_json(fmt: str, keywidth: int) -> None:
    if fmt == "json" and keywidth != 1:
        raise ValueError("the json interface cannot hold a list under a key of width %d" % keywidth)


def _free(comps) -> None:
    for a in comps:
        a.free()


def _members_or_none(comps):
    if comps is not None and not all(a.isMember() for a in comps):
        _free(comps)
        return None
    return comps


def _write_file(path: str, data) -> None:
    with open(path, "wb") as f:
        f.write(data)


def _parse_list(call, shape, grp, text, expected_n: int, report: Optional[dict], ncomp: int) -> Optional[List[PGroupElementArray]]:
    """A ciphertext list through ``call(grp, *shape, text, len, expected_n, arrays, lines, format_ok, first_bad_line,
    all_in_range)``: its ``ncomp`` arrays, or ``None`` on a format defect, a value out of range or a non-member."""
    blk = host_block(text) or host_block(bytes(text))
    hs = (C.c_void_p * ncomp)()
    n, bad = C.c_size_t(0), C.c_size_t(0)
    fmt, rng = C.c_int(0), C.c_int(1)
    _check(call(grp._h, *[C.c_size_t(s) for s in shape], blk[0], C.c_size_t(blk[1]), C.c_size_t(expected_n), hs, C.byref(n),
                C.byref(fmt), C.byref(bad), C.byref(rng)))
    if report is not None:
        report.update(format_ok=bool(fmt.value), first_bad_line=bad.value, all_in_range=bool(rng.value), lines=n.value)
    if not fmt.value:
        return None
    comps = [PGroupElementArray(grp, C.c_void_p(h)) for h in hs]
    if not rng.value:
        _free(comps)
        return None
    return _members_or_none(comps)


def parse_native(grp, text, width: int, expected_n: int = 0, report: Optional[dict] = None,
                 keywidth: int = 1) -> Optional[List[PGroupElementArray]]:
    """The 2w component arrays ``u_1..u_w, v_1..v_w`` of a native list held in memory (``bytes``, or a host buffer object as
    ``host_block`` takes them); ``None`` when a line is malformed, a value is out of range or an element is no member of the
    group -- the raw reader's policy.  ``report`` (a dict) receives ``format_ok``, ``first_bad_line`` (zero-based; only
    meaningful when ``format_ok`` is false), ``all_in_range`` and ``lines``.  Under a key of width ``keywidth`` = kappa the
    2 kappa w arrays in flat order, component l kappa + j the key j of plaintext component l."""
    return _parse_list(lib().vmn_garrays_from_hexlines_keyed, (keywidth, width), grp, text, expected_n, report, 2 * keywidth * width)


def format_native(comps: Sequence[PGroupElementArray], keywidth: int = 1) -> bytes:
    """The native text of a list given as its 2w component arrays (2 kappa w under a key of width ``keywidth``): lowercase
    digits, every line ended by a newline."""
    width = len(comps) // (2 * keywidth) if keywidth >= 1 else 0
    if width < 1 or len(comps) != 2 * keywidth * width:
        raise ValueError("a ciphertext list has 2 * keywidth * width component arrays")
    hs = (C.c_void_p * len(comps))(*[a._h for a in comps])
    size = lib().vmn_garrays_hexlines_size_keyed(hs, C.c_size_t(keywidth), C.c_size_t(width))
    out = C.create_string_buffer(max(1, size))
    _check(lib().vmn_garrays_to_hexlines_keyed(hs, C.c_size_t(keywidth), C.c_size_t(width), out))
    return out.raw[:size]


def json_max_line_bytes(grp, width: int) -> int:
    """The longest json ciphertext line over ``grp`` at ``width``, newline included (0 over a curve group)."""
    return lib().vmn_jsonlines_max_line_bytes(grp._h, C.c_size_t(width))


def parse_json(grp, text, width: int, expected_n: int = 0, report: Optional[dict] = None) -> Optional[List[PGroupElementArray]]:
    """``parse_native`` for a json list: the 2w component arrays, or ``None`` under the same policy, with the same ``report``
    keys.  A curve group raises (the json interface covers modular groups only, as the reference's)."""
    return _parse_list(lib().vmn_garrays_from_jsonlines, (width,), grp, text, expected_n, report, 2 * width)


def _json_lines(comps: Sequence[PGroupElementArray], width: int, plain: bool) -> bytes:
    if not comps:
        raise ValueError("no arrays")
    grp, n = comps[0].group, comps[0].size()
    hs = (C.c_void_p * len(comps))(*[a._h for a in comps])
    cap = max(1, n * json_max_line_bytes(grp, width))
    out = C.create_string_buffer(cap)
    written = C.c_size_t(0)
    call = lib().vmn_garrays_to_jsonplain if plain else lib().vmn_garrays_to_jsonlines
    _check(call(hs, C.c_size_t(width), out, C.c_size_t(cap), C.byref(written)))
    return out.raw[:written.value]


def format_json(comps: Sequence[PGroupElementArray]) -> bytes:
    """The json text of a list given as its 2w component arrays, exactly as the reference writes it."""
    width = len(comps) // 2
    if width < 1 or len(comps) != 2 * width:
        raise ValueError("a ciphertext list has 2 * width component arrays")
    return _json_lines(comps, width, False)


def format_json_plaintexts(comps: Sequence[PGroupElementArray]) -> bytes:
    """The json text of a list of plaintexts given as its w component arrays: line i is ``"M"`` or ``["M1",...,"Mw"]``."""
    return _json_lines(comps, len(comps), True)


def read_ciphertexts(grp, path: str, width: int, fmt: str = "native", expected_n: int = 0,
                     report: Optional[dict] = None, keywidth: int = 1) -> Optional[List[PGroupElementArray]]:
    """The list file at ``path`` in the interface ``fmt``; ``None`` when it is missing or is no such list."""
    if fmt not in FORMATS:
        raise ValueError("unknown interface %r (native, raw)" % (fmt,))
    if fmt == "raw":
        return _members_or_none(proofdir.read_ciphertexts(grp, path, width, expected_n, keywidth))
    buf = proofdir._read_file(path)
    if buf is None:
        return None
    return parse_native(grp, buf, width, expected_n, report, keywidth)


def write_ciphertexts(path: str, comps: Sequence[PGroupElementArray], fmt: str = "native", keywidth: int = 1) -> None:
    if fmt not in FORMATS:
        raise ValueError("unknown interface %r (native, raw)" % (fmt,))
    if fmt == "raw":
        proofdir.write_ciphertexts(path, comps, keywidth)
        return
    _write_file(path, format_native(comps, keywidth))


def read_plaintexts(grp, path: str, width: int, keywidth: int = 1) -> Optional[List[PGroupElementArray]]:
    """The w component arrays of a raw list of plaintexts (what the mix-net leaves behind: one array tree at width 1, the node of
    w array trees above; under a key of width kappa the kappa w arrays of ``proofdir``'s nested form); ``None`` when the file is
    missing or is no such list -- format, range and membership as for a list of ciphertexts."""
    buf = proofdir._read_file(path)
    if buf is None:
        return None
    return _members_or_none(proofdir.read_array_nests(grp, bytes(buf), 1, width, keywidth))


def write_plaintexts(path: str, comps: Sequence[PGroupElementArray], fmt: str = "json", keywidth: int = 1) -> None:
    """decodePlaintexts: the list of plaintexts given as its w component arrays, as ``json`` lines or ``raw`` -- the array tree
    as it is (ProtocolElGamalInterfaceRaw.java:93-96): one array at width 1, the node of the w arrays above, nested once more
    under a key of width ``keywidth`` (``raw`` only)."""
    if fmt not in PLAINTEXT_FORMATS:
        raise ValueError("unknown plaintext interface %r (%s)" % (fmt, ", ".join(PLAINTEXT_FORMATS)))
    _no_keyed_json(fmt, keywidth)
    if not comps:
        raise ValueError("no arrays")
    if fmt == "json":
        data = format_json_plaintexts(comps)
    else:
        data = proofdir._wide_array_tree(comps, keywidth)
    _write_file(path, data)


def convert_ciphertexts(grp, src: str, dst: str, width: int, in_fmt: str, out_fmt: str, report: Optional[dict] = None,
                        keywidth: int = 1) -> bool:
    """``vmnc -ciphs -ini in_fmt -outi out_fmt src dst``: False (and no output file) when ``src`` is no list of ``in_fmt``."""
    comps = read_ciphertexts(grp, src, width, in_fmt, report=report, keywidth=keywidth)
    if comps is None:
        return False
    try:
        write_ciphertexts(dst, comps, out_fmt, keywidth)
    finally:
        _free(comps)
    return True


# ---- all three interfaces ---------------------------------------------------------------------------------------------------------
# read_ciphertexts / write_ciphertexts / convert_ciphertexts keep the two interfaces they were written for: that any other name,
# "json" among them, is a ValueError there is their contract (tests/test_gpu_hexlines.py).  These three take every interface of
# INTERFACES under the same policy -- a format defect, a value out of range or a non-member is no list.
def read_list(grp, path: str, width: int, fmt: str, expected_n: int = 0, report: Optional[dict] = None,
              keywidth: int = 1) -> Optional[List[PGroupElementArray]]:
    """The list file at ``path`` in the interface ``fmt`` (native, raw, json); ``None`` when it is missing or is no such list."""
    if fmt not in INTERFACES:
        raise ValueError("unknown interface %r (%s)" % (fmt, ", ".join(INTERFACES)))
    _no_keyed_json(fmt, keywidth)
    if fmt != "json":
        return read_ciphertexts(grp, path, width, fmt, expected_n, report, keywidth)
    buf = proofdir._read_file(path)
    if buf is None:
        return None
    return parse_json(grp, buf, width, expected_n, report)


def write_list(path: str, comps: Sequence[PGroupElementArray], fmt: str, keywidth: int = 1) -> None:
    if fmt not in INTERFACES:
        raise ValueError("unknown interface %r (%s)" % (fmt, ", ".join(INTERFACES)))
    _no_keyed_json(fmt, keywidth)
    if fmt != "json":
        write_ciphertexts(path, comps, fmt, keywidth)
        return
    _write_file(path, format_json(comps))


def convert_list(grp, src: str, dst: str, width: int, in_fmt: str, out_fmt: str, report: Optional[dict] = None,
                 keywidth: int = 1) -> bool:
    """``vmnc -ciphs -ini in_fmt -outi out_fmt src dst`` over all three interfaces: False (and no output file) when ``src`` is no
    list of ``in_fmt``."""
    if out_fmt not in INTERFACES:
        raise ValueError("unknown interface %r (%s)" % (out_fmt, ", ".join(INTERFACES)))
    _no_keyed_json(out_fmt, keywidth)
    comps = read_list(grp, src, width, in_fmt, report=report, keywidth=keywidth)
    if comps is None:
        return False
    try:
        write_list(dst, comps, out_fmt, keywidth)
    finally:
        _free(comps)
    return True


# ---- the public key of the json interface: four numbers, on the host -------------------------------------------------------------
def write_public_key_json(path: str, p: int, q: int, g: int, y: int, encoding: Optional[int] = None) -> None:
    """``{"g":..,"p":..,"q":..,"y":..,"encoding":..}`` with decimal strings (ProtocolElGamalInterfaceJSON.java:110-126).
    ``encoding``: VCR's ModPGroup encoding scheme; by default 1 for a safe prime (p = 2q + 1), else 2."""
    if encoding is None:
        encoding = 1 if p == 2 * q + 1 else 2
    text = json.dumps({"g": str(g), "p": str(p), "q": str(q), "y": str(y), "encoding": str(encoding)}, separators=(",", ":"))
    with open(path, "w") as f:
        f.write(text)


def _decimal(value) -> int:
    if not isinstance(value, str) or not value.isascii() or not value.isdigit():
        raise ValueError("not an unsigned decimal string: %r" % (value,))
    return int(value)


def read_public_key_json(path: str) -> dict:
    """``{"p", "q", "g", "y", "encoding"}`` as integers (ProtocolElGamalInterfaceJSON.java:151-206).  The file needs at least p, q,
    g and y; without "encoding" it is 1 when p = 2q + 1, else 2; y must lie in the group.  ``ValueError`` otherwise."""
    with open(path) as f:
        try:
            obj = json.load(f)
        except ValueError as e:
            raise ValueError("no json public key: %s" % e)
    if not isinstance(obj, dict):
        raise ValueError("no json public key: not a map")
    missing = [k for k in ("p", "q", "g", "y") if k not in obj]
    if missing:
        raise ValueError("no json public key: %s missing" % ", ".join(missing))
    p, q, g, y = (_decimal(obj[k]) for k in ("p", "q", "g", "y"))
    encoding = _decimal(obj["encoding"]) if "encoding" in obj else (1 if p == 2 * q + 1 else 2)
    if not (p > 2 and q > 1 and (p - 1) % q == 0 and 1 < g < p and pow(g, q, p) == 1):
        raise ValueError("no json public key: p, q, g are no group")
    if not (0 < y < p and pow(y, q, p) == 1):
        raise ValueError("no json public key: y is not in the group")
    return {"p": p, "q": q, "g": g, "y": y, "encoding": encoding}


# ---- plaintexts as text: messages encoded as group elements (csrc/encode_layout.h) ------------------------------------------------
def encode_length(grp) -> int:
    """L: the bytes of a message one element of ``grp`` holds (``pGroup.getEncodeLength()``): floor((bits(p) - 2) / 8) - 4 over a
    modular group with p = 2q + 1; 0 over every other group, which ``encode_texts`` / ``decode_texts`` refuse."""
    return lib().vmn_group_encode_length(grp._h)


def encode_texts(grp, text, ncomp: int = 1, report: Optional[dict] = None) -> Optional[List[PGroupElementArray]]:
    """The ``ncomp`` arrays that hold the lines of ``text`` (``bytes`` or a host buffer object), line i cut into pieces of
    ``encode_length`` bytes over the components of element i; ``None`` when a line has more than ncomp * L bytes.  Lines end
    with \\n, \\r or \\r\\n; an empty line is the empty message.  ``report`` receives ``fits``, ``first_long_line``
    (zero-based; only meaningful when ``fits`` is false) and ``lines``."""
    return _encode_lines(lib().vmn_garrays_from_textlines, grp, text, ncomp, report)


def _encode_lines(call, grp, text, ncomp: int, report: Optional[dict]) -> Optional[List[PGroupElementArray]]:
    blk = host_block(text) or host_block(bytes(text))
    hs = (C.c_void_p * ncomp)()
    n, long_line, fits = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    _check(call(grp._h, C.c_size_t(ncomp), blk[0], C.c_size_t(blk[1]), hs, C.byref(n), C.byref(fits), C.byref(long_line)))
    if report is not None:
        report.update(fits=bool(fits.value), first_long_line=long_line.value, lines=n.value)
    if not fits.value:
        return None
    return [PGroupElementArray(grp, C.c_void_p(h)) for h in hs]


def _decode_lines(call, length, comps: Sequence[PGroupElementArray], report: Optional[dict]) -> bytes:
    """``length(grp)``: the bytes of a message one element holds, for the size of the buffer."""
    if not comps:
        raise ValueError("no arrays")
    grp, n = comps[0].group, comps[0].size()
    hs = (C.c_void_p * len(comps))(*[a._h for a in comps])
    cap = max(1, n * (len(comps) * length(grp) + 1))
    out = C.create_string_buffer(cap)
    written, wf, utf8 = C.c_size_t(0), C.c_int(1), C.c_int(1)
    _check(call(hs, C.c_size_t(len(comps)), out, C.c_size_t(cap), C.byref(written), C.byref(wf), C.byref(utf8)))
    if report is not None:
        report.update(all_wellformed=bool(wf.value), all_utf8=bool(utf8.value))
    return out.raw[:written.value]


def decode_texts(comps: Sequence[PGroupElementArray], report: Optional[dict] = None) -> bytes:
    """decodePlaintexts: one line per element -- the messages of its components one after the other, \\n and \\r removed, then
    \\n.  ``report`` receives ``all_wellformed`` (no element without a message: such a one gives an empty piece) and
    ``all_utf8`` (every line well-formed UTF-8 before the removal; a line that is not is written byte for byte)."""
    return _decode_lines(lib().vmn_garrays_to_textlines, encode_length, comps, report)


def write_decoded_plaintexts(path: str, comps: Sequence[PGroupElementArray]) -> None:
    """``vmnc -plain -outi native``: the list of plaintexts given as its component arrays, as lines of text."""
    _write_file(path, decode_texts(comps))


def read_texts(grp, path: str, ncomp: int, report: Optional[dict] = None) -> Optional[List[PGroupElementArray]]:
    """The lines of the file at ``path`` as ``ncomp`` arrays; ``None`` when it is missing or a line does not fit."""
    buf = proofdir._read_file(path)
    if buf is None:
        return None
    return encode_texts(grp, buf, ncomp, report)


def demo_texts(n: int, ncomp_L: int) -> bytes:
    """The reference's dummy messages (ProtocolElGamalInterfaceString.java:315-372) for elements that hold ``ncomp_L`` bytes: line
    i is the decimal i zero-padded to the full encode length when ``len(str(n))`` fits it, else the letter chr(65 + i % 26)."""
    if len(str(n)) <= ncomp_L:
        return b"".join(b"%0*d\n" % (ncomp_L, i) for i in range(n))
    return b"".join(b"%c\n" % (65 + i % 26) for i in range(n))


def demo_ciphertexts(grp, y, n: int, rand, width: int = 1) -> List[PGroupElementArray]:
    """demoCiphertexts (:374-428): the ``n`` dummy messages encrypted under the key (g, ``y``): u = g^r, v = y^r encode(text), the
    exponents from ``rand`` (``ring_array(n)``, once per component).  Returns the 2 * width arrays u_1..u_w, v_1..v_w."""
    return _demo_ciphertexts(encode_texts, encode_length, grp, y, n, rand, width)


def _demo_ciphertexts(encode, length, grp, y, n: int, rand, width: int) -> List[PGroupElementArray]:
    msgs = encode(grp, demo_texts(n, width * length(grp)), width)
    if msgs is None:
        raise ValueError("the group holds no message")
    us, vs = [], []
    for m in msgs:
        r = grp.ringArray(rand.ring_array(n))
        t = grp.exp(y, r)
        us.append(grp.exp(grp.g, r))
        vs.append(t.mul(m))
        for a in (r, t, m):
            a.free()
    return us + vs


# ---- the same over curve groups: messages as points (csrc/ec_encode_layout.h) ----------------------------------------------------------
def point_encode_length(grp) -> int:
    """L over a curve group: floor((bits(p) - 2) / 8) - 5 for the field prime p (26 over P-256); 0 over a modular group, which
    ``encode_point_texts`` / ``decode_point_texts`` refuse."""
    return lib().vmn_ec_group_encode_length(grp._h)


def encode_point_texts(grp, text, ncomp: int = 1, report: Optional[dict] = None) -> Optional[List[PGroupElementArray]]:
    """``encode_texts`` over a curve group: line i is cut into pieces of ``point_encode_length`` bytes, each the x coordinate of a
    point under the least counter that puts it on the curve (``vmn_ec_arrays_from_textlines``).  ``None`` when a line has more
    than ncomp * L bytes; ``report`` receives ``fits``, ``first_long_line`` and ``lines``."""
    return _encode_lines(lib().vmn_ec_arrays_from_textlines, grp, text, ncomp, report)


def decode_point_texts(comps: Sequence[PGroupElementArray], report: Optional[dict] = None) -> bytes:
    """``decode_texts`` over a curve group (``vmn_ec_arrays_to_textlines``): the message of a point is read from its x coordinate;
    ``report`` receives ``all_wellformed`` and ``all_utf8``."""
    return _decode_lines(lib().vmn_ec_arrays_to_textlines, point_encode_length, comps, report)


def write_decoded_point_plaintexts(path: str, comps: Sequence[PGroupElementArray]) -> None:
    """``vmnc -plain -outi native`` of a curve session: the list of plaintexts given as its component arrays, as lines of text."""
    _write_file(path, decode_point_texts(comps))


def read_point_texts(grp, path: str, ncomp: int, report: Optional[dict] = None) -> Optional[List[PGroupElementArray]]:
    """The lines of the file at ``path`` as ``ncomp`` arrays of points; ``None`` when it is missing or a line does not fit."""
    buf = proofdir._read_file(path)
    if buf is None:
        return None
    return encode_point_texts(grp, buf, ncomp, report)


def demo_point_ciphertexts(grp, y, n: int, rand, width: int = 1) -> List[PGroupElementArray]:
    """``demo_ciphertexts`` over a curve group: the ``n`` dummy messages of ``demo_texts`` as points, encrypted under (g, ``y``).
    Returns the 2 * width arrays u_1..u_w, v_1..v_w."""
    return _demo_ciphertexts(encode_point_texts, point_encode_length, grp, y, n, rand, width)
