"""lio_grid_filter_expression without a GPU: the compiler (lio_grid_expression_check) and the program run on the host
(lio_debug_grid_expression_host, the header text the kernels run) against the independent numpy restatement of EigenLab's
passes (tests/grid_expression_restate.py) on the case lists of tests/grid_expression_cases.py.  Exact cases are compared word
for word with the NaN masks equal (a NaN's sign and payload are the platform's); the transcendentals and pow, which the host
runs through libm and the restatement through numpy, at one float32 step -- two doubles that differ by far less than a float32
step round, monotonically, to the same or adjacent floats."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_expression_cases as K                              # noqa: E402
import grid_expression_restate as R                            # noqa: E402

SHAPES = ((1, 1), (1, 7), (7, 1), (5, 4))


def restated(expression, names, layers):
    """names: {variable: layer id}; layers: [n, rows, cols]"""
    return R.evaluate(expression, {k: layers[i] for k, i in names.items()})


def host(pkg, expression, names, layers):
    """the debug entry takes the layers in the order of the names"""
    order = sorted(names, key=names.get)
    return pkg.grid_expression_host(expression, order, np.stack([layers[names[k]] for k in order]))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_exact_cases_equal_the_restatement_word_for_word(pkg, rows, cols):
    layers = K.layers(rows, cols)
    for expression, names in K.EXACT:
        want, exact, _ = restated(expression, names, layers)
        assert exact, expression
        got = host(pkg, expression, names, layers)
        assert R.same_words(got, want), (expression, got, want)


def test_inputs_carry_every_special_value():
    z = K.layers(5, 4)
    assert np.isnan(z).any() and (z == np.inf).any() and (z == -np.inf).any()
    assert ((z == 0) & ~np.signbit(z)).any() and ((z == 0) & np.signbit(z)).any()
    assert ((z != 0) & (np.abs(z) < np.finfo(np.float32).tiny)).any()


def test_transcendentals_and_pow_within_one_float_step_of_the_restatement(pkg):
    layers = K.unit_layers(5, 4)
    for expression, names in K.INEXACT:
        want, exact, _ = restated(expression, names, layers)
        assert not exact, expression
        got = host(pkg, expression, names, layers)
        worst, n = R.ulps(got, want)
        assert worst <= 1, (expression, worst, n)


def test_the_quirks_of_the_passes(pkg):
    a, b, c = (np.full((2, 2), v, np.float32) for v in (3.0, 2.0, 0.5))
    layers = np.stack([a, b, c])

    def run(e):
        return host(pkg, e, K.NAMES, layers)[0, 0]
    assert run("-a^2") == 9.0                                  # negation before powers
    assert run("a.^b.^c") == 3.0 and run("a^2^3") == 729.0     # (a ^ b) ^ c
    assert run("a - b + c") == 1.5 and run("a - b - c") == 0.5 and run("a / 2 * 4") == 6.0
    assert run("2^-1 * a") == 1.5 and run("a - -b") == 5.0
    assert run("1e-3 * a") == np.float32(1e-3) * np.float32(3.0) and run("a*1.5e+1-b") == 43.0
    assert run("abs (a - 5)") == 2.0
    log = np.full((2, 2), 7.0, np.float32)                     # a layer named like a function is the layer
    assert host(pkg, "log + a", {"a": 0, "log": 1}, np.stack([a, log]))[0, 0] == 10.0


def test_self_test_expressions_equal_direct_numpy_arithmetic(pkg):
    rng = np.random.default_rng(5)
    a, b = (rng.uniform(-1, 1, (3, 4)).astype(np.float32) for _ in range(2))     # Derived::Random(3, 4)
    assert {e["expression"] for e in K.GOLDEN["self_test"]} == set(K.SELF_TEST)
    for entry in K.GOLDEN["self_test"]:
        e = entry["expression"]
        with np.errstate(all="ignore"):
            want = K.SELF_TEST[e](a, b).astype(np.float32)
        got = host(pkg, K.with_literal_s(e), {"a": 0, "b": 1}, np.stack([a, b]))
        if e in K.SELF_TEST_EXACT:
            assert R.same_words(got, want), (entry, got, want)
        else:
            assert R.ulps(got, want)[0] <= 1, (entry, got, want)
    for entry in K.GOLDEN["self_test_scalar"]:
        with pytest.raises(pkg.LioError, match="yields a scalar"):
            pkg.grid_expression_check(K.with_literal_s(entry["expression"]), {"a": 0, "b": 1})


def test_the_reference_files_expressions(pkg):
    for group in ("yaml", "readme"):
        for entry in K.GOLDEN[group]:
            names = {n: k for k, n in enumerate(entry["names"])}
            layers = K.unit_layers(4, 3, n=len(names))
            want, exact, _ = restated(entry["expression"], names, layers)
            got = host(pkg, entry["expression"], names, layers)
            assert R.same_words(got, want) if exact else R.ulps(got, want)[0] <= 1, entry
    for group in ("yaml_scalar", "readme_scalar"):             # a 1 x 1 result: refused (a labelled deviation)
        for entry in K.GOLDEN[group]:
            with pytest.raises(pkg.LioError, match="yields a scalar"):
                pkg.grid_expression_check(entry["expression"], {n: k for k, n in enumerate(entry["names"])})
    for entry in K.GOLDEN["yaml_refused"]:
        with pytest.raises(pkg.LioError, match="matrix literal"):
            pkg.grid_expression_check(entry["expression"], {n: k for k, n in enumerate(entry["names"])})


def test_info_equals_what_the_restatement_counts(pkg):
    layers = K.layers(3, 2)
    for expression, names in K.EXACT + K.INEXACT:
        _, _, p = restated(expression, names, layers)
        info = pkg.grid_expression_check(expression, names)
        bits = sum(1 << names[n] for n in p.layers_read)
        assert (info["n_passes"], info["layers_read"], info["stack_depth"], info["n_ops"]) == (p.n_passes, bits, p.stack_depth, p.n_ops), expression
        assert info["rows"] == info["cols"] == info["n_finite"] == 0
    deep = pkg.grid_expression_check(K.chain(16), K.NAMES)
    assert deep["stack_depth"] == 16 and deep["n_ops"] == 31
    assert pkg.grid_expression_check("a" + " + a" * 63, K.NAMES)["n_ops"] == 127
    assert pkg.grid_expression_check("a" + " - meanOfFinites(a)" * 8, K.NAMES)["n_passes"] == 9
    # a listed name the expression does not read costs nothing
    assert pkg.grid_expression_check("b", {"a": 0, "b": 9, "c": 15})["layers_read"] == 1 << 9


def test_the_restatement_refuses_what_the_library_refuses(pkg):
    lib = pkg.load_library()
    layers = K.layers(3, 2)
    for expression, names, code, part, key in K.REFUSED:
        with pytest.raises(R.Refused) as e:
            restated(expression, names, layers)
        assert e.value.key == key, (expression, e.value.key, key)
        keys = [k.encode() for k in names]
        rc = lib.lio_grid_expression_check(expression.encode(), (C.c_char_p * len(keys))(*keys), (C.c_int32 * len(keys))(*names.values()), len(keys), None)
        assert rc == code and part in lib.lio_last_error().decode(), (expression, rc, lib.lio_last_error())


def test_out_may_be_an_input_of_the_host_entry(pkg):
    lib = pkg.load_library()
    z = np.ascontiguousarray(K.layers(4, 3)[0].ravel(order="F"))
    want = host(pkg, "a - meanOfFinites(a)", {"a": 0}, z.reshape(1, 3, 4).transpose(0, 2, 1))
    keys = (C.c_char_p * 1)(b"a")
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.lio_debug_grid_expression_host(b"a - meanOfFinites(a)", keys, 1, p, 4, 3, p) == 0
    assert R.same_words(z.reshape(3, 4).T, want)
