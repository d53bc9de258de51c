"""GPU suite: what the four text interfaces launch (verificatum_vmn_amd/interface.py: parse_native / format_native, unkeyed and
under a key of width 2, parse_json / format_json / format_json_plaintexts, encode_texts / decode_texts, encode_point_texts /
decode_point_texts).  Every call runs under the context's timing and its launches per kernel family are compared, by equality,
with the literals of TABLE below: the host code around the kernels may be rearranged, what runs on the device may not.

TABLE is measured, not derived: it is the output of measure_*() on the commit before the interfaces were put behind one
reader and one writer skeleton (gather() prints it), and launch counts are deterministic.  (`k_u32_scan_top` is launched
outside the timed launcher and is in no family.)

Groups: the smallest of the interfaces' own suites -- the 512-bit golden group, P-256 at the reference's coordinates for
`native`, P-192 for the point texts --, at width 1 and 2.  Sizes: 0, 1, the most lines whose text fits one chunk of the line
discovery and one line more; for the readers also that last text with a line spoilt and with an expected count off by one.

Wall time on an MI355X (one run): the four cases 0.8 s together, set-up included."""
import os
import re

import pytest

from conftest import ROOT, load_golden

from named_curves import ref_curve

pytestmark = pytest.mark.gpu

POOL = 41


def chunk_bytes():
    """Bytes of text per workgroup of the line discovery, as the source states them."""
    csrc = os.path.join(ROOT, "verificatum-vmn_amd", "csrc")
    block = int(re.search(r"constexpr int BLOCK = (\d+);", open(os.path.join(csrc, "modp_kernels.h")).read()).group(1))
    seg = int(re.search(r"constexpr int HEXLINES_SEG = (\d+);", open(os.path.join(csrc, "light_kernels.h")).read()).group(1))
    return block * seg


def counted(ctx, fn):
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        out = fn()
        return out, {name: row[0] for name, row in ctx.timing_report().items() if row[0]}
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()


def free(arrays):
    for a in arrays or []:
        a.free()


def lines_of(text):
    return [l + b"\n" for l in text.split(b"\n")[:-1]]


def sizes(lines):
    """{label: N}: no line, one, the most of `lines` that fit one chunk, and one more."""
    chunk, total, fit = chunk_bytes(), 0, 0
    for l in lines:
        total += len(l)
        if total > chunk:
            break
        fit += 1
    assert 1 < fit < len(lines), "the sample is too short to need a second chunk"
    return {"none": 0, "one": 1, "one-chunk": fit, "two-chunks": fit + 1}


def modp512(vmn, ctx):
    from oracle import pyref
    g, _ = load_golden(512)
    p = g["p"]
    return vmn.ModPGroup(ctx, p, g["q"], g["g"]), [pow(2 + v % (p - 3), 2, p) for v in pyref.stream_ints(b"text-launches", POOL, p)]


def p256(vmn, ctx):
    c, acc, pool = ref_curve("P-256"), None, []
    for _ in range(POOL):
        acc = c.add(acc, c.g)
        pool.append(acc)
    return vmn.ECqPGroup(ctx, "P-256", java_widths=True), pool


def upload(G, pool, ncomp, n):
    if n == 0:
        return [G.toElementArray(b"") for _ in range(ncomp)]
    return [G.toElementArray([pool[(5 * i + 11 * c) % POOL] for i in range(n)]) for c in range(ncomp)]


def measure_lists(ctx, G, pool, tag, ncomp, nmax, fmt, parse):
    """One list interface at one shape: fmt(comps) -> text, parse(text, expected_n) -> arrays | None."""
    got = {}
    full = upload(G, pool, ncomp, nmax)
    lines = lines_of(fmt(full))
    free(full)
    for label, n in sizes(lines).items():
        comps = upload(G, pool, ncomp, n)
        text, got["format/%s/%s" % (tag, label)] = counted(ctx, lambda: fmt(comps))
        assert text == b"".join(lines[:n])
        back, got["parse/%s/%s" % (tag, label)] = counted(ctx, lambda: parse(text, 0))
        assert back is not None and len(back) == ncomp and back[0].size() == n
        free(comps + back)
    spoilt = b"".join(lines[:n // 2] + [lines[n // 2][:-2] + b"\n"] + lines[n // 2 + 1:n])
    back, got["parse/%s/bad-line" % tag] = counted(ctx, lambda: parse(spoilt, 0))
    assert back is None
    back, got["parse/%s/count-off-by-one" % tag] = counted(ctx, lambda: parse(text, n + 1))
    assert back is None
    return got


def measure_native(vmn, ctx, interface):
    got = {}
    for name, make in (("modp512", modp512), ("P-256", p256)):
        G, pool = make(vmn, ctx)
        for kw in (1, 2):
            for w in (1, 2):
                got.update(measure_lists(ctx, G, pool, "%s/kw%d/w%d" % (name, kw, w), 2 * kw * w, 40,
                                         lambda comps: interface.format_native(comps, keywidth=kw),
                                         lambda text, expected: interface.parse_native(G, text, w, expected, keywidth=kw)))
        G.close()
    return got


def measure_json(vmn, ctx, interface):
    got = {}
    G, pool = modp512(vmn, ctx)
    for w in (1, 2):
        got.update(measure_lists(ctx, G, pool, "modp512/w%d" % w, 2 * w, 40, interface.format_json,
                                 lambda text, expected: interface.parse_json(G, text, w, expected)))
        full = upload(G, pool, w, 100)
        lines = lines_of(interface.format_json_plaintexts(full))
        free(full)
        for label, n in sizes(lines).items():
            comps = upload(G, pool, w, n)
            text, got["format-plaintexts/modp512/w%d/%s" % (w, label)] = counted(ctx, lambda: interface.format_json_plaintexts(comps))
            assert text == b"".join(lines[:n])
            free(comps)
    G.close()
    return got


def measure_texts(ctx, G, tag, L, encode, decode):
    """Messages of ten bytes a line, one line too long for the spoilt text."""
    got = {}
    lines = [b"vote %04d\n" % i for i in range(500)]
    for ncomp in (1, 2):
        for label, n in sizes(lines).items():
            text = b"".join(lines[:n])
            comps, got["encode/%s/w%d/%s" % (tag, ncomp, label)] = counted(ctx, lambda: encode(G, text, ncomp))
            assert comps is not None and len(comps) == ncomp and comps[0].size() == n
            back, got["decode/%s/w%d/%s" % (tag, ncomp, label)] = counted(ctx, lambda: decode(comps))
            assert back == text
            free(comps)
        spoilt = b"".join(lines[:n // 2] + [b"x" * (ncomp * L + 1) + b"\n"] + lines[n // 2 + 1:n])
        comps, got["encode/%s/w%d/long-line" % (tag, ncomp)] = counted(ctx, lambda: encode(G, spoilt, ncomp))
        assert comps is None
    return got


def measure_modp_texts(vmn, ctx, interface):
    G, _ = modp512(vmn, ctx)
    try:
        return measure_texts(ctx, G, "modp512", interface.encode_length(G), interface.encode_texts, interface.decode_texts)
    finally:
        G.close()


def measure_point_texts(vmn, ctx, interface):
    G = vmn.ECqPGroup(ctx, "P-192")
    try:
        return measure_texts(ctx, G, "P-192", interface.point_encode_length(G), interface.encode_point_texts, interface.decode_point_texts)
    finally:
        G.close()


MEASURES = {"native": measure_native, "json": measure_json, "texts": measure_modp_texts, "point-texts": measure_point_texts}


def gather(vmn, ctx):
    """The whole table as this tree gives it (how TABLE was taken)."""
    from verificatum_vmn_amd import interface
    return {name: fn(vmn, ctx, interface) for name, fn in MEASURES.items()}


def sized(tag, launches, **refusals):
    """The rows of one call at one shape: nothing at N = 0, `launches` at the three other sizes (the measured rows did not
    differ among them), and the refusals of a reader."""
    rows = {tag + "/none": {}, tag + "/one": launches, tag + "/one-chunk": launches, tag + "/two-chunks": launches}
    rows.update({"%s/%s" % (tag, name.replace("_", "-")): counts for name, counts in refusals.items()})
    return rows


HEX_REFUSALS = dict(bad_line={"hexlines": 5}, count_off_by_one={"hexlines": 3})
JSON_REFUSALS = dict(bad_line={"jsonlines": 5}, count_off_by_one={"jsonlines": 3})
TABLE = {
    "native": {
        **sized("format/modp512/kw1/w1", {"export": 2, "hexlines": 1}),
        **sized("format/modp512/kw1/w2", {"export": 4, "hexlines": 1}),
        **sized("format/modp512/kw2/w1", {"export": 4, "hexlines": 1}),
        **sized("format/modp512/kw2/w2", {"export": 8, "hexlines": 1}),
        **sized("format/P-256/kw1/w1", {"export": 2, "hexlines": 1}),
        **sized("format/P-256/kw1/w2", {"export": 4, "hexlines": 1}),
        **sized("format/P-256/kw2/w1", {"export": 4, "hexlines": 1}),
        **sized("format/P-256/kw2/w2", {"export": 8, "hexlines": 1}),
        **sized("parse/modp512/kw1/w1", {"hexlines": 5, "import": 2, "member": 2}, **HEX_REFUSALS),
        **sized("parse/modp512/kw1/w2", {"hexlines": 5, "import": 4, "member": 4}, **HEX_REFUSALS),
        **sized("parse/modp512/kw2/w1", {"hexlines": 5, "import": 4, "member": 4}, **HEX_REFUSALS),
        **sized("parse/modp512/kw2/w2", {"hexlines": 5, "import": 8, "member": 8}, **HEX_REFUSALS),
        **sized("parse/P-256/kw1/w1", {"hexlines": 5, "import": 2}, **HEX_REFUSALS),       # (isMember launches nothing over a curve)
        **sized("parse/P-256/kw1/w2", {"hexlines": 5, "import": 4}, **HEX_REFUSALS),
        **sized("parse/P-256/kw2/w1", {"hexlines": 5, "import": 4}, **HEX_REFUSALS),
        **sized("parse/P-256/kw2/w2", {"hexlines": 5, "import": 8}, **HEX_REFUSALS),
    },
    "json": {
        **sized("format/modp512/w1", {"export": 2, "jsonlines": 4}),
        **sized("format/modp512/w2", {"export": 4, "jsonlines": 4}),
        **sized("format-plaintexts/modp512/w1", {"export": 1, "jsonlines": 4}),
        **sized("format-plaintexts/modp512/w2", {"export": 2, "jsonlines": 4}),
        **sized("parse/modp512/w1", {"import": 2, "jsonlines": 6, "member": 2}, **JSON_REFUSALS),
        **sized("parse/modp512/w2", {"import": 4, "jsonlines": 6, "member": 4}, **JSON_REFUSALS),
    },
    "texts": {
        **sized("encode/modp512/w1", {"encode_residue": 1, "import": 1, "textlines": 5}, long_line={"textlines": 5}),
        **sized("encode/modp512/w2", {"encode_residue": 2, "import": 2, "textlines": 5}, long_line={"textlines": 5}),
        **sized("decode/modp512/w1", {"export": 1, "textlines": 4}),
        **sized("decode/modp512/w2", {"export": 2, "textlines": 4}),
    },
    "point-texts": {
        **sized("encode/P-192/w1", {"encode_root": 1, "encode_search": 1, "textlines": 5}, long_line={"textlines": 5}),
        **sized("encode/P-192/w2", {"encode_root": 2, "encode_search": 2, "textlines": 5}, long_line={"textlines": 5}),
        **sized("decode/P-192/w1", {"export": 1, "textlines": 4}),
        **sized("decode/P-192/w2", {"export": 2, "textlines": 4}),
    },
}


@pytest.mark.parametrize("name", list(MEASURES))
def test_every_call_launches_what_it_launched_before_the_skeletons(vmn, gpu_ctx, name):
    from verificatum_vmn_amd import interface
    before = gpu_ctx.memory_stats()["live_bytes"]
    got = MEASURES[name](vmn, gpu_ctx, interface)
    assert sorted(got) == sorted(TABLE[name])
    differing = {k: (got[k], TABLE[name][k]) for k in got if got[k] != TABLE[name][k]}
    assert not differing, differing
    assert gpu_ctx.memory_stats()["live_bytes"] == before
