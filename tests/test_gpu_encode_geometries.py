"""GPU suite: the residue fix of the message encoding (csrc/modp_kernels.h: k_jacobi_fix, k_jacobi_fix_lanes) in EVERY geometry
it is instantiated in, 256 to 16384 bits -- tests/test_gpu_textlines.py runs the golden groups, 512 to 4096 bits.  The moduli are
those of the Jacobi edge catalogue (tests/jacobi_edges.py): all ones and a seeded N = 3 mod 8, composite, which the library takes
with q = (N - 1) / 2; the symbol decides as it does under a prime, and a value that shares a factor with N (symbol 0) stays.
Expected: the value of encode_cases.value_of, negated when the textbook symbol is -1; and the text comes back."""
import pytest

import encode_cases as ec
import jacobi_edges as je

pytestmark = pytest.mark.gpu

CASES = [(geo.id, name) for geo in je.GEOMETRIES for name in ("ones", "rnd3")]


@pytest.mark.parametrize("geo_id,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_the_fix_follows_the_symbol_in_every_geometry(vmn, gpu_ctx, geo_id, name):
    from verificatum_vmn_amd import interface
    geo = je.GEOMETRY[geo_id]
    N = je.modulus(geo, name)
    assert N % 4 == 3
    G = vmn.ModPGroup(gpu_ctx, N, (N - 1) // 2, 3, nbytes=geo.bits // 8)
    try:
        L = ec.encode_length(N)
        assert interface.encode_length(G) == L >= 1
        n = 24 if geo.bits >= 8192 else 70                      # (the textbook symbol takes ~45 ms a value at 16384 bits)
        lines = [ec.line_safe(ec.stream(b"geometries/%d/%d" % (geo.bits, i), (i * 37) % (L + 1))) for i in range(n - 3)]
        lines += [b"", b"\x01", b"\xff" * L]
        text = b"".join(ln + b"\n" for ln in lines)
        symbols = [je.jacobi(ec.value_of(ln, L), N) for ln in lines]
        assert {1, -1} <= set(symbols)
        want = [v if s != -1 else N - v for v, s in ((ec.value_of(ln, L), s) for ln, s in zip(lines, symbols))]
        arrays = interface.encode_texts(G, text)
        assert arrays[0].toBytes() == b"".join(v.to_bytes(geo.bits // 8, "big") for v in want)
        report = {}
        assert interface.decode_texts(arrays, report) == text and report["all_wellformed"]
        arrays[0].free()
    finally:
        G.close()
