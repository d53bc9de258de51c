"""The safe-prime message encoding and the text interface behind a session, restated on Python integers
(csrc/encode_layout.h, csrc/encode_kernels.h; csrc/vmnhip.hip: vmn_group_encode_length / vmn_garrays_from_textlines /
vmn_garrays_to_textlines).  Never calls the library.  Shared by tests/test_encode_catalogue.py (the restatement checks itself; no
GPU), tests/test_encode_layout_host.py (the header as host code against it) and tests/test_gpu_textlines.py (the kernels
against it, by exact equality).

The rule: b = bits(p), L = (b - 2) // 8 - 4; T = be32(|m|) || m || zeros on L + 4 bytes (|m| = 0: T[4] = 1); v = int(T); the
element is v when (v / p) = 1, else p - v.  decode: v = min(e, p - e); ill-formed (empty message) when v >= 2^(8 (L + 4)) or the
length word exceeds L.  Several components: pieces of L bytes, the later ones empty; decoding concatenates.  A decoded line is
the concatenation without its 0x0A and 0x0D bytes, then \\n; UTF-8 is judged before the removal."""
import functools
import hashlib

GROUP_BITS = (512, 1024, 2048, 3072, 4096)
ENCODE_LENGTH = {512: 59, 1024: 123, 2048: 251, 3072: 379, 4096: 507}
NS = (0, 1, 2, 63, 64, 65, 257, 1000)
NCOMPS = (1, 2, 3)


def encode_length(p: int) -> int:
    return max(0, (p.bit_length() - 2) // 8 - 4)


def jacobi(a: int, n: int) -> int:
    """(a / n) for odd n > 0, by the binary algorithm's rules."""
    a %= n
    t = 1
    while a:
        while a % 2 == 0:
            a //= 2
            if n % 8 in (3, 5):
                t = -t
        a, n = n, a
        if a % 4 == 3 and n % 4 == 3:
            t = -t
        a %= n
    return t if n == 1 else 0


def value_of(piece: bytes, L: int) -> int:
    assert len(piece) <= L
    T = bytearray(len(piece).to_bytes(4, "big") + piece + bytes(L - len(piece)))
    if not piece:
        T[4] = 1
    return int.from_bytes(T, "big")


@functools.lru_cache(maxsize=None)         # (a text of a thousand lines repeats its pieces: one Jacobi symbol each)
def encode_piece(piece: bytes, p: int) -> int:
    v = value_of(piece, encode_length(p))
    return v if jacobi(v, p) == 1 else p - v


def pieces(msg: bytes, ncomp: int, L: int):
    assert len(msg) <= ncomp * L
    return [msg[c * L:(c + 1) * L] for c in range(ncomp)]


def encode_message(msg: bytes, p: int, ncomp: int = 1):
    """The ncomp elements of one message."""
    return [encode_piece(piece, p) for piece in pieces(msg, ncomp, encode_length(p))]


def decode_element(e: int, p: int):
    """(message, well-formed)"""
    q, L = (p - 1) // 2, encode_length(p)
    v = e if e <= q else p - e
    if v >= 1 << (8 * (L + 4)):
        return b"", False
    T = v.to_bytes(L + 4, "big")
    n = int.from_bytes(T[:4], "big")
    if n > L:
        return b"", False
    return T[4:4 + n], True


def utf8_wellformed(data: bytes) -> bool:
    """Unicode table 3-7, byte by byte (the test compares it with bytes.decode)."""
    need, lo, hi = 0, 0x80, 0xBF
    for b in data:
        if need == 0:
            lo, hi = 0x80, 0xBF
            if b < 0x80:
                continue
            if 0xC2 <= b <= 0xDF:
                need = 1
            elif 0xE0 <= b <= 0xEF:
                need = 2
                lo = 0xA0 if b == 0xE0 else lo
                hi = 0x9F if b == 0xED else hi
            elif 0xF0 <= b <= 0xF4:
                need = 3
                lo = 0x90 if b == 0xF0 else lo
                hi = 0x8F if b == 0xF4 else hi
            else:
                return False
        else:
            if not lo <= b <= hi:
                return False
            need -= 1
            lo, hi = 0x80, 0xBF
    return need == 0


def decode_line(elements, p: int):
    """(the line with its \\n, all well-formed, utf-8) of the ncomp elements of one list entry."""
    parts = [decode_element(e, p) for e in elements]
    whole = b"".join(m for m, _ in parts)
    return whole.replace(b"\n", b"").replace(b"\r", b"") + b"\n", all(ok for _, ok in parts), utf8_wellformed(whole)


def decode_text(columns, p: int):
    """(text, all_wellformed, all_utf8) of ncomp columns of n integers each."""
    lines = [decode_line(row, p) for row in zip(*columns)]
    return b"".join(t for t, _, _ in lines), all(w for _, w, _ in lines), all(u for _, _, u in lines)


def split_lines(text: bytes):
    """Lines as Java's readLine ends them: \\n, \\r, \\r\\n once; text behind the last terminator is a line if not empty."""
    out, cur, i = [], bytearray(), 0
    while i < len(text):
        b = text[i]
        if b in (0x0A, 0x0D):
            out.append(bytes(cur))
            cur = bytearray()
            if b == 0x0D and i + 1 < len(text) and text[i + 1] == 0x0A:
                i += 1
        else:
            cur.append(b)
        i += 1
    if cur:
        out.append(bytes(cur))
    return out


def encode_text(text: bytes, p: int, ncomp: int):
    """(columns | None, first long line): ncomp columns of integers, or None and the zero-based index of the first line
    that has more than ncomp L bytes."""
    L = encode_length(p)
    lines = split_lines(text)
    for i, line in enumerate(lines):
        if len(line) > ncomp * L:
            return None, i
    rows = [encode_message(line, p, ncomp) for line in lines]
    return [[row[c] for row in rows] for c in range(ncomp)], 0


def demo_texts(n: int, ncomp_L: int) -> bytes:
    if len(str(n)) <= ncomp_L:
        return b"".join(str(i).rjust(ncomp_L, "0").encode() + b"\n" for i in range(n))
    return b"".join(bytes([65 + i % 26]) + b"\n" for i in range(n))


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
def stream(tag: bytes, n: int) -> bytes:
    out, ctr = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(tag + ctr.to_bytes(8, "big")).digest()
        ctr += 1
    return bytes(out[:n])


def line_safe(data: bytes) -> bytes:
    """The same bytes without line terminators (a message that is to survive as ONE line of an input text)."""
    return bytes(0x2E if b in (0x0A, 0x0D) else b for b in data)


def lengths(L: int, ncomp: int):
    """0, 1, L - 1, L, L + 1, ncomp L - 1, ncomp L -- those that fit ncomp components."""
    return sorted({k for k in (0, 1, L - 1, L, L + 1, ncomp * L - 1, ncomp * L) if 0 <= k <= ncomp * L})


EURO, G_CLEF, E_ACUTE = "€".encode(), "\U0001d11e".encode(), "é".encode()          # 3, 4 and 2 bytes


def messages(L: int, ncomp: int):
    """Messages without line terminators (each is one line of a text): every length of lengths() with random bytes, all 0x00,
    all 0xff; a lone 0x01; 2-, 3- and 4-byte characters, one of each straddling a component boundary where there is one."""
    out = []
    for k in lengths(L, ncomp):
        out += [line_safe(stream(b"encode-cases/%d/%d" % (L, k), k)), bytes(k), b"\xff" * k]
    out += [b"\x01", E_ACUTE + EURO + G_CLEF, ("grüße €5 \U0001d11e" * 3).encode()[:ncomp * L]]
    if ncomp > 1:
        for ch in (E_ACUTE, EURO, G_CLEF):
            out.append(b"a" * (L - 1) + ch + b"z")             # the character's first byte ends component 0
    out.append(b"A" * (L - 2) + G_CLEF[:2] if ncomp == 1 else b"A" * (L - 2) + G_CLEF)          # (cut off at width 1: not UTF-8)
    return out


def sample_text(L: int, ncomp: int, n: int, tag: bytes = b"") -> bytes:
    """n lines drawn round-robin from messages() (every one of them from n = len(messages()) on), ended by \\n."""
    pool = messages(L, ncomp)
    return b"".join(pool[(i + len(tag)) % len(pool)] + b"\n" for i in range(n))


# payloads for the decoder that no input text produces (built by value_of / raw integers)
BAD_UTF8 = (b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"abc\xe2\x82", b"\x80", b"ok\xffok")
STRIPPED = (b"\nabc", b"abc\r", b"a\nb\rc", b"\r\n", b"\n", b"x\r\ny\n")
C3_0A_A9 = b"\xc3\x0a\xa9"                                     # not UTF-8 before the removal, written as C3 A9


def ill_formed_values(p: int):
    """Members' folded values v that hold no message: length words L + 1, 2^31, 0xffffffff, and v >= 2^(8 (L + 4))."""
    L = encode_length(p)
    tail = stream(b"ill-formed", L)
    out = [int.from_bytes(n.to_bytes(4, "big") + tail, "big") for n in (L + 1, 1 << 31, 0xffffffff)]
    out.append((1 << (8 * (L + 4))) + 5)
    return out


def member_of(v: int, p: int) -> int:
    """v or p - v, whichever is in the group (0 < v < p)."""
    return v if jacobi(v, p) == 1 else p - v


# ---- a modular group that is no safe-prime group: 512-bit p = k q + 1, k > 2 --------------------------------------------------------
def is_probable_prime(n: int) -> bool:
    if n < 2:
        return False
    for s in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % s == 0:
            return n == s
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def search_cofactor_group(seed: bytes = b"encode-cases/cofactor"):
    """The first 256-bit prime q, then the first even k for which p = k q + 1 is a 512-bit prime, both counted up from the seed's
    hash; g = 2^k mod p."""
    q = int.from_bytes(hashlib.sha256(seed + b"/q").digest(), "big") | (3 << 254) | 1            # (top two bits set: k q has 512 bits)
    while not is_probable_prime(q):
        q += 2
    k = (int.from_bytes(hashlib.sha256(seed + b"/k").digest(), "big") | (3 << 254)) & ~1
    while not ((k * q + 1).bit_length() == 512 and is_probable_prime(k * q + 1)):
        k += 2
    p = k * q + 1
    g = pow(2, k, p)
    assert g != 1 and pow(g, q, p) == 1
    return p, q, g


COFACTOR_P = int("ae0ca5ed3cd7472180af0396d661d8337a9dcc00567d190f73a9e574cd41e3b39f2fed45636a2fbe0bffee7673b3cc976fcbefdfedeec5e4ee1be177bbf51405", 16)
COFACTOR_Q = int("e2dcc64293a06edac7fc5547ccf9c102e28a2c1d04da76e518ae9920a9cecdeb", 16)
COFACTOR_G = int("34764e98754ee4741c4e98cb59dfbeb9653fb57e342ff8cf94ef59d3c70a2bbb96b28fbb315aa25c3bb1f2f8213528e226b13c1edb212d593267e750f386674b", 16)
