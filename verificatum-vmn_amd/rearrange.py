"""rearrange.py — the reference's ``vre``: split, join and re-key public keys, lists of ciphertexts and lists of plaintexts.

Mirrors ``ProtocolElGamalRearParser`` (the grammar of intervals, positions, formats and widths), ``ProtocolElGamalRear`` (the
operations on arrays) and the file handling of ``ProtocolElGamalRearTool`` under protocol/elgamal/ of the reference.  Three layers:

grammar   ``parse_interval``, ``parse_intervals``, ``parse_positions``, ``parse_source``, ``parse_format``, ``parse_widths``.  They
          restate the Java, not a tidied grammar (ProtocolElGamalRearParser.java:53-299): ``String.split`` drops trailing empty
          strings and keeps leading and inner ones, so ``"0-1:"`` is one interval, ``"1-2-"`` is the interval [1, 2) and ``"-1-2"``
          is malformed; ``":"`` is no interval at all but, as a format, the empty format; a position string has at least five
          characters.  A number is what ``Integer.parseInt`` reads: an optional sign and ASCII digits, a value below 2^31.
          [NOT-IN-REF] Java also takes the digits of other scripts; this code does not.  Python's ``int()`` is never used bare: it
          takes blanks and underscores.  The reference's messages are the text of a ``RearrangeFormatError``.

plan      pure functions on integers.  A list is what ``proofdir.read_array_nests`` returns: kappa * omega component arrays per
          nest, component c = l * kappa + j, the u nest before the v nest for ciphertexts.  A plan names, for every component
          array of every output, the (input, component) it is.
          ``plan_shallow`` (rearrangeArrays / rearrangeCiphs, ProtocolElGamalRear.java:199-213, 387-419): inputs i of widths w_i
          under one keywidth kappa; position (i, j) is the kappa arrays [j kappa, (j + 1) kappa) of input i; an output of
          positions P has width |P|; the halves of ciphertexts are rearranged separately by the same format.
          ``plan_deep`` (rearrangeArraysDeep / expandPositions, :297-375): inputs i of one width w under keywidths kappa_i;
          output o has width w and keywidth |P_o|, its array (l, m) is array l * kappa_s + j of input s, (s, j) = P_o[m].
          [NOT-IN-REF] the reference builds this for plaintexts and leaves ``-deep -ciphs`` as a commented-out block that exits
          0 (ProtocolElGamalRearTool.java:993-1007); here ciphertexts follow the rule of the shallow level, each half by the same plan.
          ``plan_pkeys`` (rearrangePkeys, ProtocolElGamalRearTool.java:88-125): key i has the rows g_(i,0..kappa_i-1) and then
          y_(i,0..kappa_i-1); output o has the g rows, then the y rows, of its positions.
          [NOT-IN-REF: the reference leaves these to VCR's PGroupUtil] a position whose source or index does not exist, inputs of
          different lengths and a count of outputs that differs from the format's are a ``RearrangeFormatError``.

device    ``sub_arrays``, ``cat_arrays``, ``rearrange_shallow``, ``rearrange_deep``, ``rearrange_pkeys`` on device arrays; every
          result is a new array which the caller frees, as the inputs.  All of them are ``grp.fromSegments``
          (``vmn_garray_from_segments``, one launch per output array).
files     ``sub_files``, ``cat_files``, ``shallow_files``, ``deep_files``, ``pkeys_files`` in the raw interface, as the reference's
          tool.  Inputs are read with ``proofdir.read_array_nests`` and membership-checked as ``interface.read_ciphertexts`` does;
          an input that is missing, is no tree of the stated shape or holds a non-member raises ``RearrangeInputError`` naming
          the file, and no output file is created.  ``-shallow`` and ``-deep`` write the plan's arrays as they are: no device copy.
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence, Tuple

from . import fiatshamir as fs

INT_MAX = 2 ** 31 - 1

Position = Tuple[int, int]          # (source, index): ProtocolElGamalRearPosition
Interval = Tuple[int, int]          # [start, end): ProtocolElGamalRearInterval


class RearrangeFormatError(ValueError):
    """ProtocolFormatException of the reference's parser and operations; the text is the reference's message."""


class RearrangeInputError(Exception):
    """An input file is missing, is no tree of the stated shape, or holds an element outside the group."""

    def __init__(self, path: str, what: str):
        super().__init__("%s: %s" % (path, what))
        self.path = path


# ---- grammar ----------------------------------------------------------------------------------------------------------------
class _NumberFormat(Exception):
    """NumberFormatException."""


_JAVA_INT = re.compile(r"[+-]?[0-9]+")


def java_split(s: str, sep: str) -> List[str]:
    """``s.split(sep)`` of Java for a literal separator: no match gives [s] (also for the empty string); otherwise trailing empty
    strings are dropped, leading and inner ones kept."""
    parts = s.split(sep)
    if len(parts) == 1:
        return parts
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def parse_int(s: str) -> int:
    """``Integer.parseInt``: an optional sign, ASCII digits, a value in [-2^31, 2^31)."""
    if _JAVA_INT.fullmatch(s) is None:
        raise _NumberFormat(s)
    v = int(s)
    if not -INT_MAX - 1 <= v <= INT_MAX:
        raise _NumberFormat(s)
    return v


def parse_interval(s: str) -> Interval:
    """"s-e" with 0 <= s < e (:53-78)."""
    e = "Malformed interval! (" + s + ")"
    try:
        bounds = java_split(s, "-")
        if len(bounds) != 2:
            raise RearrangeFormatError(e)
        start, end = parse_int(bounds[0]), parse_int(bounds[1])
    except _NumberFormat:
        raise RearrangeFormatError(e) from None
    if start < 0 or start >= end:
        raise RearrangeFormatError(e)
    return start, end


def parse_intervals(s: str) -> List[Interval]:
    """"A:B:C" (:89-107)."""
    parts = java_split(s, ":")
    if not parts:
        raise RearrangeFormatError("No interval is given!")
    return [parse_interval(p) for p in parts]


def _interval_to_sequence(s: str) -> List[int]:
    """"s-e" as its integers, or the single integer "s" (:119-149).  A string holding a '-' goes to parse_interval, so a negative
    single integer is a malformed interval."""
    if "-" not in s:
        try:
            return [parse_int(s)]
        except _NumberFormat:
            raise RearrangeFormatError("Malformed interval! (" + s + ")") from None
    start, end = parse_interval(s)
    return list(range(start, end))


def parse_positions(s: str, strict: bool = False) -> List[Position]:
    """"(x,y)", x and y an integer or an interval: the positions row-major (:164-208).  strict: x and y are single indices."""
    e = "Malformed position string! (" + s + ")"
    if len(s) < 5 or s[0] != "(" or s[-1] != ")":
        raise RearrangeFormatError(e)
    coeffs = java_split(s[1:-1], ",")
    if len(coeffs) != 2:
        raise RearrangeFormatError(e)
    rows = _interval_to_sequence(coeffs[0])
    columns = _interval_to_sequence(coeffs[1])
    if strict:
        if len(rows) != 1:
            raise RearrangeFormatError(e + " Invalid index! (" + coeffs[0] + ")")
        if len(columns) != 1:
            raise RearrangeFormatError(e + " Invalid index! (" + coeffs[1] + ")")
    return [(r, c) for r in rows for c in columns]


def parse_source(s: str) -> List[Position]:
    """"AxBxC" (:223-235)."""
    res: List[Position] = []
    for part in java_split(s, "x"):
        res += parse_positions(part, False)
    return res


def parse_format(s: str) -> List[List[Position]]:
    """"A:B:C", one source per output (:251-264).  ":" is the empty format."""
    return [parse_source(part) for part in java_split(s, ":")]


def parse_widths(s: str) -> List[int]:
    """"2:1:5" (:274-299)."""
    parts = java_split(s, ":")
    if not parts:
        raise RearrangeFormatError("No widths!")
    widths = []
    for part in parts:
        try:
            w = parse_int(part)
        except _NumberFormat:
            raise RearrangeFormatError("Failed to parse width! (" + part + ")") from None
        if w < 1:
            raise RearrangeFormatError("Non-positive width!")
        widths.append(w)
    return widths


# ---- plans ------------------------------------------------------------------------------------------------------------------
def _check_outputs(fmt: Sequence[Sequence[Position]], outputs: Optional[int]) -> None:
    if outputs is not None and outputs != len(fmt):
        raise RearrangeFormatError("The format (%d outputs) and the number of outputs (%d) do not match!" % (len(fmt), outputs))


def _check_position(pos: Position, limits: Sequence[int], what: str) -> None:
    s, j = pos
    if not 0 <= s < len(limits):
        raise RearrangeFormatError("Position (%d,%d) names source %d of %d!" % (s, j, s, len(limits)))
    if not 0 <= j < limits[s]:
        raise RearrangeFormatError("Position (%d,%d) names index %d of a source of %s %d!" % (s, j, j, what, limits[s]))


def plan_shallow(widths: Sequence[int], keywidth: int, fmt: Sequence[Sequence[Position]], ciphs: bool,
                 outputs: Optional[int] = None) -> List[List[Position]]:
    """For every output the (input, component) of each of its component arrays, in the list's own order."""
    if keywidth < 1 or any(w < 1 for w in widths):
        raise RearrangeFormatError("Non-positive width!")
    _check_outputs(fmt, outputs)
    plan = []
    for positions in fmt:
        for pos in positions:
            _check_position(pos, widths, "width")
        half = [(i, j * keywidth + t) for i, j in positions for t in range(keywidth)]
        plan.append(half + [(i, keywidth * widths[i] + c) for i, c in half] if ciphs else half)
    return plan


def plan_deep(keywidths: Sequence[int], width: int, fmt: Sequence[Sequence[Position]], ciphs: bool,
              outputs: Optional[int] = None) -> List[List[Position]]:
    """plan_shallow's counterpart one level down: output o lies under a key of width len(fmt[o])."""
    if width < 1 or any(k < 1 for k in keywidths):
        raise RearrangeFormatError("Non-positive width!")
    _check_outputs(fmt, outputs)
    plan = []
    for positions in fmt:
        for pos in positions:
            _check_position(pos, keywidths, "keywidth")
        half = [(s, l * keywidths[s] + j) for l in range(width) for s, j in positions]
        plan.append(half + [(s, width * keywidths[s] + c) for s, c in half] if ciphs else half)
    return plan


def plan_pkeys(keywidths: Sequence[int], fmt: Sequence[Sequence[Position]], outputs: Optional[int] = None) -> List[List[Position]]:
    """Key i as its 2 kappa_i rows (g rows, then y rows): for every output the (key, row) of its g rows, then of its y rows."""
    return plan_deep(keywidths, 1, fmt, True, outputs)


# ---- operations on device lists -----------------------------------------------------------------------------------------------
def _free(arrays) -> None:
    for a in arrays:
        a.free()


def _same_length(inputs: Sequence[Sequence]) -> int:
    sizes = [a.size() for comps in inputs for a in comps]
    if len(set(sizes)) > 1:
        raise RearrangeFormatError("The input arrays differ in length! (%s)" % ", ".join(str(comps[0].size()) for comps in inputs if comps))
    return sizes[0] if sizes else 0


def _check_intervals(intervals: Sequence[Interval], size: int) -> None:
    """All intervals against the array's size before anything is made (ProtocolElGamalRear.java:440-451)."""
    for s, e in intervals:
        if e > size:
            raise RearrangeFormatError("Interval out of bounds! %d-%d. Length of array is %d!" % (s, e, size))


def sub_arrays(comps: Sequence, intervals: Sequence[Interval]) -> List[List]:
    """subArrays (:430-461) of a list given as its component arrays: one list per interval.  Intervals may intersect."""
    _check_intervals(intervals, _same_length([comps]))
    outs: List[List] = []
    try:
        for s, e in intervals:
            outs.append([])
            for a in comps:
                outs[-1].append(a.group.fromSegments([a], [s], [e]))
    except Exception:
        _free(a for out in outs for a in out)
        raise
    return outs


def cat_arrays(lists: Sequence[Sequence]) -> List:
    """catArrays (:469-473): lists of one width and keywidth, one after the other; a list may be empty."""
    if not lists:
        raise RearrangeFormatError("Too few files! (0)")
    if len(set(len(comps) for comps in lists)) > 1:
        raise RearrangeFormatError("The input arrays differ in width!")
    out: List = []
    try:
        for c in range(len(lists[0])):
            out.append(lists[0][c].group.concat([comps[c] for comps in lists]))
    except Exception:
        _free(out)
        raise
    return out


def _copies(inputs: Sequence[Sequence], plan: Sequence[Sequence[Position]]) -> List[List]:
    for i, comps in enumerate(inputs):
        for _, c in (p for out in plan for p in out if p[0] == i):
            if c >= len(comps):
                raise RearrangeFormatError("Input %d has %d component arrays, the plan names component %d!" % (i, len(comps), c))
    outs: List[List] = []
    try:
        for positions in plan:
            outs.append([])
            for i, c in positions:
                outs[-1].append(inputs[i][c].group.concat([inputs[i][c]]))
    except Exception:
        _free(a for out in outs for a in out)
        raise
    return outs


def rearrange_shallow(inputs: Sequence[Sequence], widths: Sequence[int], keywidth: int, fmt, ciphs: bool) -> List[List]:
    """rearrangeArrays / rearrangeCiphs on device lists of one length: copies of the chosen arrays, one list per output."""
    if len(inputs) != len(widths):
        raise RearrangeFormatError("The number of widths (%d) does not equal the number of inputs (%d)!" % (len(widths), len(inputs)))
    plan = plan_shallow(widths, keywidth, fmt, ciphs)
    _same_length(inputs)
    return _copies(inputs, plan)


def rearrange_deep(inputs: Sequence[Sequence], keywidths: Sequence[int], width: int, fmt, ciphs: bool) -> List[List]:
    """rearrangeArraysDeep on device lists of one length and one width."""
    if len(inputs) != len(keywidths):
        raise RearrangeFormatError("The number of public keys (%d) does not equal the number of inputs (%d)!" % (len(keywidths), len(inputs)))
    plan = plan_deep(keywidths, width, fmt, ciphs)
    _same_length(inputs)
    return _copies(inputs, plan)


def rearrange_pkeys(keys: Sequence, fmt) -> List:
    """rearrangePkeys: key i is ONE array of its 2 kappa_i rows (g rows, then y rows); every output is such an array again,
    gathered in one launch (a segment of one row per chosen row)."""
    if any(k.size() < 2 or k.size() % 2 for k in keys):
        raise RearrangeFormatError("Failed to project to part of public key!")
    plan = plan_pkeys([k.size() // 2 for k in keys], fmt)
    outs: List = []
    try:
        for rows in plan:
            outs.append(keys[rows[0][0]].group.fromSegments([keys[i] for i, _ in rows], [r for _, r in rows], [r + 1 for _, r in rows]))
    except Exception:
        _free(outs)
        raise
    return outs


# ---- operations on files (the raw interface) ----------------------------------------------------------------------------------
def pkey_keywidth(grp, buf: Optional[bytes]) -> Optional[int]:
    """The keywidth a raw public key states in the header of its first half: node(g', y), a half the tree of one element at
    kappa = 1 and node(kappa element trees) above.  None when there is no such header."""
    try:
        cur = fs.Cursor(buf or b"")
        cur.node(2)
        if grp.coord_bytes is None:                      # an element is a leaf
            return 1 if bytes(cur.buf[cur.pos:cur.pos + 1]) == b"\x01" else max(1, cur.node())
        count = cur.node()                               # an element is node(leaf(x), leaf(y))
        if bytes(cur.buf[cur.pos:cur.pos + 1]) == b"\x01":
            return 1 if count == 2 else None
        return max(1, count)
    except fs.NoSuchTree:
        return None


def _read_list(grp, path: str, width: int, keywidth: int, ciphs: bool):
    from . import proofdir
    buf = proofdir._read_file(path)
    if buf is None:
        raise RearrangeInputError(path, "no such file")
    comps = proofdir._member_arrays(proofdir.read_array_nests(grp, bytes(buf), 2 if ciphs else 1, width, keywidth))
    if comps is None:
        raise RearrangeInputError(path, "not a raw list of %s of width %d under a key of width %d over this group (format, a value "
                                  "out of range, or an element outside the group)" % ("ciphertexts" if ciphs else "plaintexts", width, keywidth))
    return comps


def _write_list(path: str, comps: Sequence, keywidth: int, ciphs: bool) -> None:
    from . import proofdir
    with open(path, "wb") as f:
        for piece in (proofdir._list_pieces(comps, keywidth) if ciphs else proofdir._nested_pieces(comps, keywidth)):
            f.write(piece)


def _read_lists(grp, paths: Sequence[str], widths: Sequence[int], keywidths: Sequence[int], ciphs: bool) -> List[List]:
    inputs: List[List] = []
    try:
        for path, w, k in zip(paths, widths, keywidths):
            inputs.append(_read_list(grp, path, w, k, ciphs))
    except Exception:
        _free(a for comps in inputs for a in comps)
        raise
    return inputs


def sub_files(grp, in_path: str, out_paths: Sequence[str], intervals: Sequence[Interval], width: int = 1, keywidth: int = 1,
              ciphs: bool = True) -> None:
    """``vre -sub -inter A:B:.. in out..`` (ProtocolElGamalRearTool.java:203-252)."""
    if len(intervals) != len(out_paths):
        raise RearrangeFormatError("Mismatching number of intervals and output filenames! (%d != %d)" % (len(intervals), len(out_paths)))
    comps = _read_list(grp, in_path, width, keywidth, ciphs)
    outs: List[List] = []
    try:
        outs = sub_arrays(comps, intervals)
        for path, out in zip(out_paths, outs):
            _write_list(path, out, keywidth, ciphs)
    finally:
        _free(comps)
        _free(a for out in outs for a in out)


def cat_files(grp, in_paths: Sequence[str], out_path: str, width: int = 1, keywidth: int = 1, ciphs: bool = True) -> None:
    """``vre -cat in.. out`` (:264-295)."""
    if not in_paths:
        raise RearrangeFormatError("Too few files! (%d)" % (len(in_paths) + 1))
    inputs = _read_lists(grp, in_paths, [width] * len(in_paths), [keywidth] * len(in_paths), ciphs)
    out: List = []
    try:
        out = cat_arrays(inputs)
        _write_list(out_path, out, keywidth, ciphs)
    finally:
        _free(a for comps in inputs for a in comps)
        _free(out)


def _write_plan(inputs, plan, out_paths, keywidths: Sequence[int], ciphs: bool) -> None:
    _same_length(inputs)
    for path, positions, k in zip(out_paths, plan, keywidths):
        _write_list(path, [inputs[i][c] for i, c in positions], k, ciphs)


def shallow_files(grp, in_paths: Sequence[str], out_paths: Sequence[str], widths: Sequence[int], keywidth: int, fmt,
                  ciphs: bool = True) -> None:
    """``vre -shallow -widths W -format F in.. out..`` (:1026-1078)."""
    if len(widths) + len(fmt) != len(in_paths) + len(out_paths) or len(widths) != len(in_paths):
        raise RearrangeFormatError("The number of widths (%d) plus the number of output files (%d) specified in the output format does not "
                                   "equal the number of filenames (%d)!" % (len(widths), len(fmt), len(in_paths) + len(out_paths)))
    plan = plan_shallow(widths, keywidth, fmt, ciphs, len(out_paths))
    inputs = _read_lists(grp, in_paths, widths, [keywidth] * len(widths), ciphs)
    try:
        _write_plan(inputs, plan, out_paths, [keywidth] * len(plan), ciphs)
    finally:
        _free(a for comps in inputs for a in comps)


def deep_files(grp, in_paths: Sequence[str], out_paths: Sequence[str], keywidths: Sequence[int], width: int, fmt,
               ciphs: bool = False) -> None:
    """``vre -deep -noin N -width W -format F`` behind its N keys (:942-1014): input i lies under a key of width keywidths[i]."""
    if len(keywidths) != len(in_paths) or len(fmt) != len(out_paths):
        raise RearrangeFormatError("The number of public keys (%d) plus the number of input group element arrays (%d) plus the number of "
                                   "output group element arrays (%d) specified in the output format does not equal the number of "
                                   "filenames (%d)!" % (len(keywidths), len(keywidths), len(fmt), len(keywidths) + len(in_paths) + len(out_paths)))
    plan = plan_deep(keywidths, width, fmt, ciphs, len(out_paths))
    inputs = _read_lists(grp, in_paths, [width] * len(keywidths), keywidths, ciphs)
    try:
        _write_plan(inputs, plan, out_paths, [len(positions) for positions in fmt], ciphs)
    finally:
        _free(a for comps in inputs for a in comps)


def read_pkey_rows(grp, path: str):
    """The 2 kappa rows (g rows, then y rows) of a raw public key file as ONE device array, membership-checked."""
    from . import native, proofdir
    buf = proofdir._read_file(path)
    if buf is None:
        raise RearrangeInputError(path, "no such file")
    kappa = pkey_keywidth(grp, buf)
    nests = proofdir._read_element_nests(grp, buf, (1, 1), kappa) if kappa is not None else None
    if nests is None:
        raise RearrangeInputError(path, "not a raw public key over this group")
    try:
        rows = grp.toElementArray(nests[0] + nests[1], checked=False)
    except (ValueError, OverflowError, native.VmnError):
        raise RearrangeInputError(path, "not a raw public key over this group") from None
    if not (rows.all_in_range and rows.isMember()):
        rows.free()
        raise RearrangeInputError(path, "the public key holds an element outside the group")
    return rows


def pkeys_files(grp, in_paths: Sequence[str], out_paths: Sequence[str], fmt) -> None:
    """``vre -pkeys -noin N -format F in.. out..`` (:139-174).  An output of one position is a plain pair: no node of width 1."""
    if len(fmt) != len(out_paths):
        raise RearrangeFormatError("The format and number of output filenames do not match!")
    keys: List = []
    outs: List = []
    try:
        for path in in_paths:
            keys.append(read_pkey_rows(grp, path))
        outs = rearrange_pkeys(keys, fmt)
        trees = [fs.product_element_tree(grp, o.toInts(), o.size() // 2) for o in outs]
        for path, tree in zip(out_paths, trees):
            with open(path, "wb") as f:
                f.write(tree)
    finally:
        _free(keys)
        _free(outs)
