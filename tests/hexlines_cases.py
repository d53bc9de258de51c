"""The native ciphertext interface in plain Python, and the catalogue of texts the GPU reader is judged on
(csrc/hexlines_layout.h, csrc/light_kernels.h: k_hexlines_count / _walk / _decode / _encode; csrc/vmnhip.hip:
vmn_garrays_from_hexlines / _to_hexlines).  Shared by tests/test_gpu_hexlines.py (the kernels against parse()),
tests/test_hexlines_catalogue.py (the catalogue holds what it claims and catches mutants of parse(); no GPU) and
tests/test_hexlines_layout_host.py (the host header against the trees built here).

A list is a text of one ciphertext per line; a line is the hex of the byte tree of that ciphertext, node(u, v), u and v element
trees at width 1 and node(w element trees) above; an element tree is leaf(value) over a modular group and
node(leaf(x), leaf(y)) over a curve.  Lines end as Java's BufferedReader.readLine ends them.

A value is the payload of its leaves: `bytes` over a modular group, a pair of `bytes` over a curve.  A row is the 2w values of
one ciphertext in the order u_1..u_w, v_1..v_w."""
import importlib.util
import os

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("hexlines_cases_eio", os.path.join(ROOT, "verificatum-vmn_amd", "eio.py"))
eio = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(eio)

HEX = frozenset(b"0123456789abcdefABCDEF")
LOWER_HEX = frozenset(b"0123456789abcdef")

# mutants of parse() (never of a kernel): what tests/test_hexlines_catalogue.py proves the catalogue catches
CRLF_TWICE, CASE_SENSITIVE, NO_LENGTH, FIRST_FOUND = "crlf-twice", "case-sensitive", "no-length-check", "first-found"
MUTANTS = (CRLF_TWICE, CASE_SENSITIVE, NO_LENGTH, FIRST_FOUND)


# ---- sizes and trees ---------------------------------------------------------------------------------------------------
def element_bytes(curve, vb):
    return 15 + 2 * vb if curve else 5 + vb


def line_bytes(curve, vb, w):
    """B: bytes of the byte tree of one ciphertext; a line has H = 2 B digits."""
    return 5 + (10 if w > 1 else 0) + 2 * w * element_bytes(curve, vb)


def element_tree(curve, value):
    return [bytes(value[0]), bytes(value[1])] if curve else bytes(value)


def ciphertext_tree(curve, w, row):
    assert len(row) == 2 * w
    parts = [[element_tree(curve, v) for v in half] for half in (row[:w], row[w:])]
    return [parts[0][0], parts[1][0]] if w == 1 else parts


def line_of(curve, w, row):
    """The digits of one ciphertext, lowercase (what the reference's own hex literals use)."""
    return eio.encode(ciphertext_tree(curve, w, row)).hex().encode("ascii")


def text_of(curve, w, rows, end=b"\n"):
    return b"".join(line_of(curve, w, r) + end for r in rows)


def component_offsets(curve, vb, w):
    """Where the 2w element trees begin inside the B bytes."""
    E = element_bytes(curve, vb)
    head = 5 + (5 if w > 1 else 0)
    return [head + c * E for c in range(w)] + [head + w * E + (5 if w > 1 else 0) + c * E for c in range(w)]


# ---- the reader ---------------------------------------------------------------------------------------------------------
def split_lines(text, mutant=None):
    """readLine until it returns null: a line ends at \\n, at \\r, or at \\r\\n, which counts once; what follows the last terminator
    is a line only if it is not empty."""
    lines, cur, i = [], bytearray(), 0
    while i < len(text):
        c = text[i]
        if c == 0x0A:
            lines.append(bytes(cur))
            cur = bytearray()
        elif c == 0x0D:
            lines.append(bytes(cur))
            cur = bytearray()
            if i + 1 < len(text) and text[i + 1] == 0x0A:
                if mutant == CRLF_TWICE:
                    lines.append(b"")
                i += 1
        else:
            cur.append(c)
        i += 1
    if cur:
        lines.append(bytes(cur))
    return lines


def _element_value(curve, vb, tree):
    if curve:
        if not (isinstance(tree, list) and len(tree) == 2 and all(isinstance(t, bytes) and len(t) == vb for t in tree)):
            raise ValueError("not node(leaf(x), leaf(y))")
        return (tree[0], tree[1])
    if not (isinstance(tree, bytes) and len(tree) == vb):
        raise ValueError("not a leaf of the group's width")
    return tree


def text_defect(line, H, mutant=None):
    """A line whose characters are not exactly H hex digits."""
    if mutant != NO_LENGTH and len(line) != H:
        return True
    return not set(line) <= (LOWER_HEX if mutant == CASE_SENSITIVE else HEX) or len(line) % 2 == 1


def decode_line(curve, vb, w, line):
    """The row of a line of hex digits, or ValueError when its bytes are not node(u, v) of this width over leaves of vb bytes."""
    tree, _ = eio.decode(bytes.fromhex(line.decode("ascii")))
    if not (isinstance(tree, list) and len(tree) == 2):
        raise ValueError("not node(u, v)")
    row = []
    for part in tree:
        if w == 1:
            row.append(_element_value(curve, vb, part))
        else:
            if not (isinstance(part, list) and len(part) == w):
                raise ValueError("not node(w elements)")
            row += [_element_value(curve, vb, t) for t in part]
    return row


def parse(text, curve, vb, w, expected_n=0, mutant=None):
    """(format_ok, first_bad_line, rows): the verdict of include/vmnhip.h on a text.  A line count that differs from a non-zero
    expected_n: (False, min(lines, expected_n), None); otherwise the smallest index of a line that has not exactly H hex
    digits or whose bytes are not the ciphertext's framing: (False, index, None); otherwise (True, 0, rows)."""
    H = 2 * line_bytes(curve, vb, w)
    lines = split_lines(bytes(text), mutant)
    if expected_n and len(lines) != expected_n:
        return False, min(len(lines), expected_n), None

    def framing_defect(line):
        try:
            decode_line(curve, vb, w, line)
            return False
        except ValueError:
            return True
    if mutant == FIRST_FOUND:                           # two passes, the first defect found is reported: not the smallest index
        for k, line in enumerate(lines):
            if text_defect(line, H):
                return False, k, None
        for k, line in enumerate(lines):
            if framing_defect(line):
                return False, k, None
    rows = []
    for k, line in enumerate(lines):
        if text_defect(line, H, mutant) or framing_defect(line):
            return False, k, None
        rows.append(decode_line(curve, vb, w, line))
    return True, 0, rows


# ---- the catalogue ----------------------------------------------------------------------------------------------------------
def positions(n):
    return sorted({0, n // 2, n - 1})


def mixed_case(line):
    return bytes(c - 32 if 0x61 <= c <= 0x66 and k % 3 == 0 else c for k, c in enumerate(line))


def valid_variants(curve, w, rows):
    """{label: text}: texts that all hold `rows`."""
    lines = [line_of(curve, w, r) for r in rows]
    ends = [b"\n", b"\r\n", b"\r"]
    out = {
        "lf": b"".join(l + b"\n" for l in lines),
        "crlf": b"".join(l + b"\r\n" for l in lines),
        "cr": b"".join(l + b"\r" for l in lines),
        "mixed": b"".join(l + ends[k % 3] for k, l in enumerate(lines)),
        "mixed-crlf-first": b"".join(l + ends[(k + 1) % 3] for k, l in enumerate(lines)),
        "no-final-terminator": b"\n".join(lines),
        "no-final-terminator-crlf": b"\r\n".join(lines),
        "upper": b"".join(l.upper() + b"\n" for l in lines),
        "mixed-case": b"".join(mixed_case(l) + b"\n" for l in lines),
    }
    return out


def _patch_byte(line, at, value):
    """The line with byte `at` of its tree replaced."""
    return line[:2 * at] + b"%02x" % value + line[2 * at + 2:]


def line_defects(curve, vb, w, line):
    """[(label, replacement lines)] for one good line: each replacement makes that line (the first of the replacement)
    defective."""
    off = component_offsets(curve, vb, w)
    leaf = off[-1] + (5 if curve else 0)                 # the header of a leaf of the last component
    last_leaf_len = leaf + 4
    out = [
        ("nonhex-first", [b"g" + line[1:]]),
        ("nonhex-last", [line[:-1] + b"G"]),
        ("nonhex-slash", [line[:7] + b"/" + line[8:]]),  # the character in front of '0'
        ("nonhex-colon", [line[:7] + b":" + line[8:]]),  # the character behind '9'
        ("nonhex-at", [line[:7] + b"@" + line[8:]]),     # in front of 'A'
        ("nonhex-backtick", [line[:7] + b"`" + line[8:]]),
        ("nonhex-high", [line[:7] + b"\xe1" + line[8:]]),
        ("one-short", [line[:-1]]),
        ("two-long", [line + b"00"]),
        ("blank", [b"", line]),
        ("space-in-front", [b" " + line]),
        ("space-behind", [line + b" "]),
        ("node-count-3", [_patch_byte(line, 4, 3)]),
        ("node-tag-1", [_patch_byte(line, 0, 1)]),
        ("leaf-tag-2", [_patch_byte(line, off[0] + (5 if curve else 0), 2)]),
        ("leaf-length+1", [_patch_byte(line, last_leaf_len, (vb + 1) & 0xff)]),
        ("leaf-length-1", [_patch_byte(line, off[0] + (5 if curve else 0) + 4, (vb - 1) & 0xff)]),
    ]
    if w > 1:
        out.append(("inner-count-2", [_patch_byte(line, 9, 2)]))
        out.append(("second-inner-count", [_patch_byte(line, off[w] - 1, w + 1)]))
    if curve:
        out.append(("point-node-count-3", [_patch_byte(line, off[0] + 4, 3)]))
    return out


def defects(curve, vb, w, rows, where=None):
    """[(label, text, first bad line)]: every defect of line_defects at the lines `where` (default: first, middle, last), a
    second terminator at the end, and pairs of defects of which the one at the smaller index must be named."""
    lines = [line_of(curve, w, r) for r in rows]
    n = len(lines)
    out = []

    def join(ls):
        return b"".join(l + b"\n" for l in ls)
    for k in (positions(n) if where is None else where):
        for label, repl in line_defects(curve, vb, w, lines[k]):
            out.append(("%s@%d" % (label, k), join(lines[:k] + repl + lines[k + 1:]), k))
    out.append(("second-terminator-at-the-end", join(lines) + b"\n", n))
    out.append(("second-terminator-at-the-end-crlf", b"".join(l + b"\r\n" for l in lines) + b"\r\n", n))
    out.append(("lf-cr-is-two-terminators", lines[0] + b"\n\r" + join(lines[1:]), 1))
    if n >= 2:
        a, b = (n - 1) // 2, n - 1
        framing = dict(line_defects(curve, vb, w, lines[a]))["node-count-3"]
        texty = dict(line_defects(curve, vb, w, lines[b]))["nonhex-first"]
        out.append(("framing@%d-before-text@%d" % (a, b), join(lines[:a] + framing + lines[a + 1:b] + texty + lines[b + 1:]), a))
        texty = dict(line_defects(curve, vb, w, lines[a]))["one-short"]
        framing = dict(line_defects(curve, vb, w, lines[b]))["leaf-tag-2"]
        out.append(("text@%d-before-framing@%d" % (a, b), join(lines[:a] + texty + lines[a + 1:b] + framing + lines[b + 1:]), a))
    return out


# ---- synthetic rows (the catalogue's own tests and the layout test need no group) ---------------------------------------------
def synthetic_rows(curve, vb, w, n, seed=1):
    """n rows of 2w values of vb bytes from a small counter-based generator; the payloads avoid nothing: a reader must not look
    into them."""
    def value(k):
        return bytes(((k * 2654435761 + j * 40503 + seed) >> 7) & 0xff for j in range(vb))
    rows = []
    for i in range(n):
        row = []
        for c in range(2 * w):
            k = (i * 2 * w + c) * 2
            row.append((value(k), value(k + 1)) if curve else value(k))
        rows.append(row)
    return rows
