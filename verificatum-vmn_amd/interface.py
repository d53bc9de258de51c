"""interface.py — the files in front of a session: ciphertext lists in the reference's two interfaces.

``raw``     one byte tree holding the 2w component arrays (``proofdir.read_ciphertexts`` / ``write_ciphertexts``): what
            the mix-net works on and what a proof directory holds.
``native``  the reference's default (``ProtocolElGamalInterfaceNative`` / ``...SeqHex``, ``CiphertextReaderLine``,
            ``CiphertextWriterLine``): one ciphertext per line, the line being the hexadecimal byte tree of that single
            ciphertext.  A ballot box delivers this; the first command of an election is ``vmnc -ciphs -ini native -outi raw``.

The native text is an array of structures, the arrays are a structure of arrays: the N lines are found, decoded, checked and
transposed on the GPU (``vmn_garrays_from_hexlines`` / ``vmn_garrays_to_hexlines``, csrc/light_kernels.h), not in a loop over
the lines.  Both readers apply one policy to what enters here from outside: a format defect, a value out of range or an
element outside the group is no list (``None``).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

from . import PGroupElementArray, _check, host_block, lib
from . import proofdir

FORMATS = ("native", "raw")


def ciphertext_line_bytes(grp, width: int) -> int:
    """B: the bytes of one ciphertext of ``width`` over ``grp`` as a byte tree; a native line has 2B hex digits."""
    return lib().vmn_hexlines_line_bytes(grp._h, C.c_size_t(width))


def _free(comps) -> None:
    for a in comps:
        a.free()


def _members_or_none(comps):
    if comps is not None and not all(a.isMember() for a in comps):
        _free(comps)
        return None
    return comps


def parse_native(grp, text, width: int, expected_n: int = 0, report: Optional[dict] = None) -> Optional[List[PGroupElementArray]]:
    """The 2w component arrays ``u_1..u_w, v_1..v_w`` of a native list held in memory (``bytes``, or a host buffer object as
    ``host_block`` takes them); ``None`` when a line is malformed, a value is out of range or an element is no member of the
    group -- the raw reader's policy.  ``report`` (a dict) receives ``format_ok``, ``first_bad_line`` (zero-based; only
    meaningful when ``format_ok`` is false), ``all_in_range`` and ``lines``."""
    blk = host_block(text) or host_block(bytes(text))
    hs = (C.c_void_p * (2 * width))()
    n, bad = C.c_size_t(0), C.c_size_t(0)
    fmt, rng = C.c_int(0), C.c_int(1)
    _check(lib().vmn_garrays_from_hexlines(grp._h, C.c_size_t(width), blk[0], C.c_size_t(blk[1]), C.c_size_t(expected_n), hs,
                                           C.byref(n), C.byref(fmt), C.byref(bad), C.byref(rng)))
    if report is not None:
        report.update(format_ok=bool(fmt.value), first_bad_line=bad.value, all_in_range=bool(rng.value), lines=n.value)
    if not fmt.value:
        return None
    comps = [PGroupElementArray(grp, C.c_void_p(h)) for h in hs]
    if not rng.value:
        _free(comps)
        return None
    return _members_or_none(comps)


def format_native(comps: Sequence[PGroupElementArray]) -> bytes:
    """The native text of a list given as its 2w component arrays: lowercase digits, every line ended by a newline."""
    width = len(comps) // 2
    if width < 1 or len(comps) != 2 * width:
        raise ValueError("a ciphertext list has 2 * width component arrays")
    hs = (C.c_void_p * len(comps))(*[a._h for a in comps])
    size = lib().vmn_garrays_hexlines_size(hs, C.c_size_t(width))
    out = C.create_string_buffer(max(1, size))
    _check(lib().vmn_garrays_to_hexlines(hs, C.c_size_t(width), out))
    return out.raw[:size]


def read_ciphertexts(grp, path: str, width: int, fmt: str = "native", expected_n: int = 0,
                     report: Optional[dict] = None) -> Optional[List[PGroupElementArray]]:
    """The list file at ``path`` in the interface ``fmt``; ``None`` when it is missing or is no such list."""
    if fmt not in FORMATS:
        raise ValueError("unknown interface %r (native, raw)" % (fmt,))
    if fmt == "raw":
        return _members_or_none(proofdir.read_ciphertexts(grp, path, width, expected_n))
    buf = proofdir._read_file(path)
    if buf is None:
        return None
    return parse_native(grp, buf, width, expected_n, report)


def write_ciphertexts(path: str, comps: Sequence[PGroupElementArray], fmt: str = "native") -> None:
    if fmt not in FORMATS:
        raise ValueError("unknown interface %r (native, raw)" % (fmt,))
    if fmt == "raw":
        proofdir.write_ciphertexts(path, comps)
        return
    text = format_native(comps)
    with open(path, "wb") as f:
        f.write(text)


def convert_ciphertexts(grp, src: str, dst: str, width: int, in_fmt: str, out_fmt: str, report: Optional[dict] = None) -> bool:
    """``vmnc -ciphs -ini in_fmt -outi out_fmt src dst``: False (and no output file) when ``src`` is no list of ``in_fmt``."""
    comps = read_ciphertexts(grp, src, width, in_fmt, report=report)
    if comps is None:
        return False
    try:
        write_ciphertexts(dst, comps, out_fmt)
    finally:
        _free(comps)
    return True
