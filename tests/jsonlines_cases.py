"""The json ciphertext interface in plain Python, and the catalogue of texts the GPU reader is judged on
(csrc/jsonlines_layout.h, csrc/decimal_kernels.h: k_jsonlines_scan / k_dec_to_rows / k_rows_to_dec / k_jsonlines_emit;
csrc/vmnhip.hip: vmn_garrays_from_jsonlines / _to_jsonlines / _to_jsonplain).  Shared by tests/test_gpu_jsonlines.py (the kernels
against parse() and the writers), tests/test_jsonlines_catalogue.py (the catalogue holds what it claims and catches mutants of
parse(); no GPU) and tests/test_jsonlines_layout_host.py (the header's tokenizer against parse()).

A list is a text of one ciphertext per line, {"alpha":"A","beta":"B"} at width 1 and an array of w such pairs above; a number is a
decimal string.  Lines end as Java's BufferedReader.readLine ends them (tests/hexlines_cases.py: split_lines).  A row is the 2w
integers of one ciphertext in the order u_1..u_w, v_1..v_w; the oracle of every value is int(str) and str(int).

The grammar of a line (BLANK = space | tab, allowed between tokens only):
    line   := pair                                   at width 1
            | '[' pair (',' pair){w-1} ']'           at width w > 1
    pair   := '{' member ',' member '}'              the two keys distinct
    member := ('"alpha"' | '"beta"') ':' '"' DIGIT+ '"'
"""
from hexlines_cases import split_lines

# mutants of parse() (never of a kernel): what tests/test_jsonlines_catalogue.py proves the catalogue catches
ORDER_SENSITIVE, NO_LEADING_ZEROS, FIRST_FOUND, EXTRA_KEY_TOLERANT = "order-sensitive", "leading-zero-refusing", "first-found", "extra-key-tolerant"
MUTANTS = (ORDER_SENSITIVE, NO_LEADING_ZEROS, FIRST_FOUND, EXTRA_KEY_TOLERANT)

PAIR_FRAMING = 22


def digits_of(p):
    """D_max: the decimal digits of p."""
    return len(str(p))


def max_line_bytes(dmax, w):
    pairs = w * (PAIR_FRAMING + 2 * dmax)
    return pairs + 1 if w == 1 else 2 + pairs + (w - 1) + 1


# ---- the writer ----------------------------------------------------------------------------------------------------------
def line_of(w, row):
    assert len(row) == 2 * w
    pairs = [b'{"alpha":"%d","beta":"%d"}' % (row[i], row[w + i]) for i in range(w)]
    return pairs[0] if w == 1 else b"[" + b",".join(pairs) + b"]"


def text_of(w, rows, end=b"\n"):
    return b"".join(line_of(w, r) + end for r in rows)


def plain_line_of(w, row):
    assert len(row) == w
    items = [b'"%d"' % v for v in row]
    return items[0] if w == 1 else b"[" + b",".join(items) + b"]"


def plain_text_of(w, rows):
    return b"".join(plain_line_of(w, r) + b"\n" for r in rows)


# ---- the reader ----------------------------------------------------------------------------------------------------------
class _Defect(Exception):
    pass


class _Cursor:
    def __init__(self, line):
        self.s, self.at = line, 0

    def blanks(self):
        while self.at < len(self.s) and self.s[self.at] in b" \t":
            self.at += 1

    def eat(self, token):
        if self.s.startswith(token, self.at):
            self.at += len(token)
            return True
        return False

    def need(self, token):
        if not self.eat(token):
            raise _Defect(token)


def _number(c, mutant):
    c.need(b'"')
    first = c.at
    while c.at < len(c.s) and 0x30 <= c.s[c.at] <= 0x39:
        c.at += 1
    run = c.s[first:c.at]
    if not run:
        raise _Defect("empty number")
    if mutant == NO_LEADING_ZEROS and len(run) > 1 and run[0] == 0x30:
        raise _Defect("leading zero")
    c.need(b'"')
    return int(run)


def _member(c, mutant):
    key = 0 if c.eat(b'"alpha"') else 1 if c.eat(b'"beta"') else None
    if key is None:
        raise _Defect("key")
    c.blanks()
    c.need(b":")
    c.blanks()
    return key, _number(c, mutant)


def _pair(c, mutant):
    c.need(b"{")
    c.blanks()
    k1, v1 = _member(c, mutant)
    c.blanks()
    c.need(b",")
    c.blanks()
    k2, v2 = _member(c, mutant)
    if k2 == k1 or (mutant == ORDER_SENSITIVE and k1 != 0):
        raise _Defect("keys")
    c.blanks()
    if mutant == EXTRA_KEY_TOLERANT:
        while c.eat(b","):
            c.blanks()
            _member(c, mutant)
            c.blanks()
    c.need(b"}")
    return (v1, v2) if k1 == 0 else (v2, v1)


def decode_line(w, line, mutant=None):
    """The row of a line, or _Defect."""
    c = _Cursor(line)
    pairs = []
    if w == 1:
        pairs.append(_pair(c, mutant))
    else:
        c.need(b"[")
        c.blanks()
        while True:
            if len(pairs) == w:
                raise _Defect("a pair too many")
            pairs.append(_pair(c, mutant))
            c.blanks()
            if not c.eat(b","):
                break
            c.blanks()
        c.need(b"]")
        if len(pairs) != w:
            raise _Defect("pair count")
    if c.at != len(line):
        raise _Defect("text behind the end")
    return [a for a, _ in pairs] + [b for _, b in pairs]


def line_defect(w, line, mutant=None):
    try:
        decode_line(w, line, mutant)
        return False
    except _Defect:
        return True


def parse(text, w, expected_n=0, mutant=None):
    """(format_ok, first_bad_line, rows): the verdict of include/vmnhip.h on a text.  A line count that differs from a non-zero
    expected_n: (False, min(lines, expected_n), None); otherwise the smallest index of a defective line: (False, index, None);
    otherwise (True, 0, rows)."""
    lines = split_lines(bytes(text))
    if expected_n and len(lines) != expected_n:
        return False, min(len(lines), expected_n), None
    if mutant == FIRST_FOUND:                           # two passes, lines of odd index first: not the smallest index
        order = list(range(1, len(lines), 2)) + list(range(0, len(lines), 2))
        for k in order:
            if line_defect(w, lines[k]):
                return False, k, None
    rows = []
    for k, line in enumerate(lines):
        if line_defect(w, line, mutant):
            return False, k, None
        rows.append(decode_line(w, line, mutant))
    return True, 0, rows


def in_range(rows, p):
    """all_in_range as vmn_garray_from_bytetree has it: every value below p (zero is in range there)."""
    return all(v < p for r in rows for v in r)


# ---- the catalogue -------------------------------------------------------------------------------------------------------
def positions(n):
    return sorted({0, n // 2, n - 1})


def _pairs_of(w, row):
    return [(row[i], row[w + i]) for i in range(w)]


def _join_pairs(w, pairs, sep=b","):
    return pairs[0] if w == 1 else b"[" + sep.join(pairs) + b"]"


def swapped_line(w, row):
    return _join_pairs(w, [b'{"beta":"%d","alpha":"%d"}' % (b, a) for a, b in _pairs_of(w, row)])


def dumps_line(w, row):
    """What json.dumps writes: ": " and ", "."""
    return _join_pairs(w, [b'{"alpha": "%d", "beta": "%d"}' % ab for ab in _pairs_of(w, row)], b", ")


def tabs_line(w, row):
    inner = _join_pairs(w, [b'{\t"alpha" \t: "%d" ,\t"beta":\t"%d" }' % ab for ab in _pairs_of(w, row)], b"\t, ")
    return inner if w == 1 else b"[ " + inner[1:-1] + b"\t]"


def zeros_line(w, row, zeros):
    z = b"0" * zeros
    return _join_pairs(w, [b'{"alpha":"' + z + b'%d","beta":"' % a + z + b'%d"}' % b for a, b in _pairs_of(w, row)])


def valid_variants(w, rows):
    """{label: text}: texts that all hold `rows`."""
    lines = [line_of(w, r) for r in rows]
    ends = [b"\n", b"\r\n", b"\r"]
    mixed = [(swapped_line, dumps_line, tabs_line, line_of)[k % 4](w, r) for k, r in enumerate(rows)]
    return {
        "lf": b"".join(l + b"\n" for l in lines),
        "crlf": b"".join(l + b"\r\n" for l in lines),
        "cr": b"".join(l + b"\r" for l in lines),
        "mixed-terminators": b"".join(l + ends[k % 3] for k, l in enumerate(lines)),
        "no-final-terminator": b"\n".join(lines),
        "no-final-terminator-crlf": b"\r\n".join(lines),
        "swapped-keys": b"".join(swapped_line(w, r) + b"\n" for r in rows),
        "json-dumps-spaces": b"".join(dumps_line(w, r) + b"\n" for r in rows),
        "tabs-and-spaces": b"".join(tabs_line(w, r) + b"\n" for r in rows),
        "leading-zeros-1": b"".join(zeros_line(w, r, 1) + b"\n" for r in rows),
        "leading-zeros-9": b"".join(zeros_line(w, r, 9) + b"\n" for r in rows),
        "leading-zeros-700": b"".join(zeros_line(w, r, 700) + b"\n" for r in rows),
        "every-variant-mixed": b"".join(l + ends[(k + 1) % 3] for k, l in enumerate(mixed[:-1])) + mixed[-1],
    }


def line_defects(w, row):
    """[(label, replacement lines)] for one good row: each replacement makes that line (the first of the replacement)
    defective."""
    line = line_of(w, row)
    a, b = row[0], row[w]
    head, tail = (b"", b"") if w == 1 else (b"[", b"]")
    rest = b"" if w == 1 else b"," + b",".join(b'{"alpha":"%d","beta":"%d"}' % ab for ab in _pairs_of(w, row)[1:])

    def first_pair(pair):                                # the line with its first pair replaced
        return head + pair + rest + tail
    da = b"%d" % a
    out = [
        ("missing-key", [first_pair(b'{"alpha":"%d"}' % a)]),
        ("missing-key-alpha", [first_pair(b'{"beta":"%d"}' % b)]),
        ("duplicate-key", [first_pair(b'{"alpha":"%d","alpha":"%d"}' % (a, b))]),
        ("duplicate-key-beta", [first_pair(b'{"beta":"%d","beta":"%d"}' % (a, b))]),
        ("unknown-key", [first_pair(b'{"alpha":"%d","gamma":"%d"}' % (a, b))]),
        ("unknown-key-case", [first_pair(b'{"Alpha":"%d","beta":"%d"}' % (a, b))]),
        ("extra-key", [first_pair(b'{"alpha":"%d","beta":"%d","gamma":"1"}' % (a, b))]),
        ("extra-key-known", [first_pair(b'{"alpha":"%d","beta":"%d","alpha":"%d"}' % (a, b, a))]),
        ("empty-number", [first_pair(b'{"alpha":"","beta":"%d"}' % b)]),
        ("sign-minus", [first_pair(b'{"alpha":"-%d","beta":"%d"}' % (a, b))]),
        ("sign-plus", [first_pair(b'{"alpha":"%d","beta":"+%d"}' % (a, b))]),
        ("non-digit-inside", [first_pair(b'{"alpha":"' + da[:1] + b"x" + da[1:] + b'","beta":"%d"}' % b)]),
        ("non-digit-slash", [first_pair(b'{"alpha":"' + da + b'/","beta":"%d"}' % b)]),
        ("non-digit-colon", [first_pair(b'{"alpha":"' + da + b':","beta":"%d"}' % b)]),
        ("space-inside-number", [first_pair(b'{"alpha":"' + da + b' ","beta":"%d"}' % b)]),
        ("hex-number", [first_pair(b'{"alpha":"0x10","beta":"%d"}' % b)]),
        ("bare-number", [first_pair(b'{"alpha":%d,"beta":"%d"}' % (a, b))]),
        ("backslash", [first_pair(b'{"alpha":"%d","beta":"\\u0031%d"}' % (a, b))]),
        ("backslash-in-key", [first_pair(b'{"al\\u0070ha":"%d","beta":"%d"}' % (a, b))]),
        ("high-byte", [first_pair(b'{"alpha":"%d","beta":"\xc2\xa0%d"}' % (a, b))]),
        ("high-byte-between-tokens", [first_pair(b'{"alpha":"%d",\xa0"beta":"%d"}' % (a, b))]),
        ("pair-count-one-more", [head + line[len(head):len(line) - len(tail)] + b',{"alpha":"1","beta":"1"}' + tail]),
        ("text-behind", [line + b"x"]),
        ("space-behind", [line + b" "]),
        ("space-in-front", [b" " + line]),
        ("second-line-behind", [line + line]),
        ("blank", [b"", line]),
        ("blank-of-spaces", [b" \t", line]),
        ("truncated", [line[:-1]]),
        ("truncated-in-number", [line[:len(head) + 12]]),
        ("newline-form-feed", [line[:-1] + b"\x0c" + line[-1:]]),
        ("nul-byte", [line[:3] + b"\x00" + line[3:]]),
        ("single-quotes", [line.replace(b'"', b"'")]),
    ]
    if w == 1:
        out.append(("list-at-width-1", [b"[" + line + b"]"]))
        out.append(("empty-map", [b"{}"]))
    else:
        pairs = [b'{"alpha":"%d","beta":"%d"}' % ab for ab in _pairs_of(w, row)]
        out.append(("bare-map-at-width-w", [pairs[0]]))
        out.append(("pair-count-one-less", [b"[" + b",".join(pairs[:-1]) + b"]"]))
        out.append(("empty-list", [b"[]"]))
        out.append(("trailing-comma", [b"[" + b",".join(pairs) + b",]"]))
        out.append(("missing-comma", [b"[" + b"".join(pairs) + b"]"]))
        out.append(("unclosed-list", [b"[" + b",".join(pairs)]))
        out.append(("nested-list", [b"[[" + b",".join(pairs) + b"]]"]))
    return out


def defects(w, rows, where=None):
    """[(label, text, first bad line)]: every defect of line_defects at the lines `where` (default: first, middle, last), each
    together with a second, later defect where there is a later line, a second terminator at the end, and pairs of defects of
    which the one at the smaller index must be named."""
    lines = [line_of(w, r) for r in rows]
    n = len(lines)
    out = []

    def join(ls):
        return b"".join(l + b"\n" for l in ls)
    for k in (positions(n) if where is None else where):
        for label, repl in line_defects(w, rows[k]):
            later = list(lines[k + 1:])
            if later:                                    # a second defect behind it: the smaller line is the one named
                later[-1] = later[-1][:-2] + b"?" + later[-1][-2:]
            out.append(("%s@%d" % (label, k), join(lines[:k] + repl + later), k))
    out.append(("second-terminator-at-the-end", join(lines) + b"\n", n))
    out.append(("second-terminator-at-the-end-crlf", b"".join(l + b"\r\n" for l in lines) + b"\r\n", n))
    out.append(("lf-cr-is-two-terminators", lines[0] + b"\n\r" + join(lines[1:]), 1))
    if n >= 3:                                           # a defect at an odd line behind one at an even line, and the reverse
        for a, b in ((n - 3, n - 2), (n - 2, n - 1)):
            ls = list(lines)
            ls[a] = dict(line_defects(w, rows[a]))["extra-key"][0]
            ls[b] = dict(line_defects(w, rows[b]))["sign-minus"][0]
            out.append(("two-defects-extra-key@%d-before-sign@%d" % (a, b), join(ls), a))
    return out


# ---- synthetic rows (the catalogue's own tests and the layout test need no group) ----------------------------------------
def synthetic_rows(w, n, digits=40, seed=1):
    """n rows of 2w integers of up to `digits` digits from a small counter-based generator; some short, one zero, one 1."""
    rows = []
    for i in range(n):
        row = []
        for c in range(2 * w):
            k = (i * 2 * w + c) * 2654435761 + seed
            v = pow(k | 1, 7, 10 ** digits)
            row.append(v % 10 ** (1 + (k >> 3) % digits) if c % 3 == 2 else v)
        rows.append(row)
    if n:
        rows[0][0] = 1
        rows[-1][-1] = 0
    return rows
