"""CPU suite: the case list of vmn_garray_expprod_arrays (tests/expprod_arrays_cases.py) itself, on Python integers and affine
points: every expected value is defined, and every situation the GPU suite has to meet is there by name."""
import expprod_arrays_cases as X


def test_every_expected_value_is_defined():
    for case in X.catalogue():
        G, xs = X.group(case["group"]), X.pool(case["group"], case["n"])
        assert len(case["bases"]) == len(case["ints"]) >= 1 and max(case["bases"]) < X.POOL, case["name"]
        for b in set(case["bases"]):
            assert len(xs[b]) == case["n"]
            if G["kind"] == "modp":
                assert all(0 < v < G["p"] for v in xs[b]), (case["name"], b)          # invertible: a negative exponent is defined
            else:
                assert all(G["curve"].on_curve(P) for P in xs[b]), (case["name"], b)
        want = X.expected(case)
        assert len(want) == case["n"]
        if not any(case["ints"]):
            assert want == [1 if G["kind"] == "modp" else None] * case["n"], case["name"]


def test_every_named_situation_is_in_the_catalogue():
    cases = X.catalogue()
    tags = set().union(*(c["tags"] for c in cases))
    for tag in X.REQUIRED_TAGS:
        assert tag in tags, tag
    L = X.launch_limit()
    by = lambda tag: [c for c in cases if tag in c["tags"]]
    assert all(len(c["ints"]) == L for c in by("k_limit")) and all(len(c["ints"]) == L + 1 for c in by("k_limit_plus_1"))
    assert all(len(c["ints"]) == 4 for c in by("k4")) and all(len(c["ints"]) == 5 for c in by("k5"))
    assert all(c["ints"] == [1] for c in by("k1_copy")) and all(c["ints"] == [-1] for c in by("k1_inverse"))
    assert any(c["ints"] == [2, -1] and c["group"] == "g14" for c in by("benchmark_2_-1"))
    assert all(min(c["ints"]) > 0 for c in by("all_positive")) and all(max(c["ints"]) < 0 for c in by("all_negative"))
    assert all(c["ints"][1] == 0 and c["ints"][0] and c["ints"][2] for c in by("zero_in_the_middle"))
    assert all(not any(c["ints"]) for c in by("all_zero"))
    assert all(any("0" * 33 in bin(abs(v)) for v in c["ints"]) for c in by("zero_run_above_32"))
    for c in by("full_length_3"):
        q = X.group(c["group"])["q"]
        assert c["n"] == 3 and len(c["ints"]) == 3 and all(abs(v).bit_length() == q.bit_length() for v in c["ints"])
    assert all(len(set(c["bases"])) < len(c["bases"]) for c in by("same_array_twice") + by("same_array_equal_exponents"))
    assert all(c["ints"][0] == c["ints"][1] and c["bases"][0] == c["bases"][1] for c in by("same_array_equal_exponents"))
    for c in by("length_gap"):
        q = X.group(c["group"])["q"]
        lens = [abs(v).bit_length() for v in c["ints"]]
        assert max(lens) - min(lens) == q.bit_length() - 1, c["name"]
    # every group kind: the four RFC 3526 groups, the subgroup fixture, both curve kinds
    assert {c["group"] for c in cases} == {"g14", "g15", "g16", "g17", "sub1024", "P-256", "P-384", "bp256"}
    assert [X.group(k)["p"].bit_length() for k in ("g14", "g15", "g16", "g17")] == [2048, 3072, 4096, 6144]
    assert X.group("sub1024")["q"] != (X.group("sub1024")["p"] - 1) // 2
    assert X.group("bp256")["curve"].a != X.group("bp256")["p"] - 3 and X.group("P-384")["curve"].a == X.group("P-384")["p"] - 3
    # elements: 1 and p - 1 among the modular bases; infinity rows, P and -P at one index over the curves
    xs = X.pool("g14", 5)
    assert xs[0][0] == 1 and xs[1][0] == X.group("g14")["p"] - 1
    for key in X.CURVES:
        xs, cur = X.pool(key, X.CURVE_N), X.group(key)["curve"]
        assert xs[0][0] is None and xs[2][-1] is None and xs[1][1] == cur.neg(xs[0][1]) and xs[0][1] is not None
        assert any({0, 1} <= set(c["bases"]) and c["group"] == key for c in by("p_and_minus_p"))
    assert {c["n"] for c in cases if c["group"] == "g14" and c["both_geometries"]} == {1, X.EPB - 1, X.EPB, X.EPB + 1}
    assert [c["n"] for c in cases if c["group"] == "g15" and c["both_geometries"]] == [65]          # the 3072-bit case too
    assert all(c["both_geometries"] for c in cases if c["group"] == "g15")
