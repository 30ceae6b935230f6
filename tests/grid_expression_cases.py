"""The case lists of lio_grid_filter_expression's tests: what is accepted (with every quirk of EigenLab's chunk passes that
include/liogpu.h promises), what is refused and why, the reference's own expression strings (tests/golden/
grid_expression_reference.json) and the layers the cases run on.  NAMES: a, b, c stand for layers 0, 1, 2."""
import json
import math
import os
import re

import numpy as np

f32 = np.float32
NAMES = {"a": 0, "b": 1, "c": 2}
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_expression_reference.json")))
S_LITERAL = "0.625"                                            # EigenLab's scalar variable s, written as a literal


def chain(n, op="+"):
    """a op (a op (a ...)) with n operands: a stack of n"""
    return ("a " + op + " (") * (n - 1) + "a" + ")" * (n - 1)


# (expression, names): every operation IEEE basic -- compared word for word
EXACT = [(e, NAMES) for e in (
    # each binary op in its three shape forms, plain and dotted
    "a + b", "a + 3", "3 + a", "a .+ b", "a .+ 3", "3 .+ a",
    "a - b", "a - 3", "3 - a", "a .- b", "a .- 3", "3 .- a",
    "a .* b", "a * 3", "3 * a", "a .* 3", "3 .* a",
    "a ./ b", "a / 3", "3 / a", "a ./ 3", "3 ./ a", "0.5 / a",
    # negation: a product with -1, before every other pass
    "-a", "-(a + b)", "a - -b", "a .* -b", "2 * -a", "-a - -b",
    # left to right within a pass
    "a - b + c", "a - b - c", "a / 2 * 3", "a .* b ./ c", "a ./ b .* c", "a - (b + c)", "a + b .* c - 1",
    # numbers through the sign-accepting scanner, and fields that are trimmed
    "1e-3 * a", "1E+2*a", "a*1.5e+1-b", "a * 1.e1", "a - 2.5e-1 + b", " a  +  b ", "a * .5", "a + 5.",
    # functions; `abs (a)` with a space is a call
    "abs(a)", "abs (a)", "sqrt(abs(a))", "sqrt(a)", "square(a - b)", "abs(a - b)",
    "cwiseMin(a, b)", "cwiseMax(a, b)", "cwiseMax(a, 0)", "cwiseMin(a, 0.5)", "cwiseMax(cwiseMin(a, 1), -1)", "cwiseMin(2, 3) * a",
    "cwiseMin(a , b - 1)", "cwiseMax(a, minOfFinites(b))",
    # parentheses and nesting
    "(a)", "((a + b))", "(a + b) .* (a - b)", "0.5 * (1.0 - (a / 0.6)) + 0.5 * (1.0 - (b / 0.1))", "square(sqrt(abs(a)) - (b ./ (c + 1)))",
    # the map-wide reductions, of a layer and of a scalar, nested
    "a - meanOfFinites(a)", "sumOfFinites(a) * b", "minOfFinites(a) + b", "maxOfFinites(a) - b", "numberOfFinites(a) .* b",
    "numberOfFinites(2) * a", "meanOfFinites(3) * a", "sumOfFinites(minOfFinites(a)) + b", "meanOfFinites(maxOfFinites(a)) + b",
    "numberOfFinites(sumOfFinites(a)) + b", "a - meanOfFinites(a - meanOfFinites(a))",
    "0 * a + sqrt(sumOfFinites(square(a - meanOfFinites(a))) ./ numberOfFinites(a))",
    "(a - minOfFinites(a)) / (maxOfFinites(a) - minOfFinites(a))", "cwiseMax(cwiseMin(a - b, maxOfFinites(c)), minOfFinites(c))",
    "sumOfFinites(abs(a .* b)) + c", "sumOfFinites(a + meanOfFinites(b)) - maxOfFinites(square(c)) + a",
    # the limits, reached
    chain(16), "a" + " + a" * 63, "a" + " - meanOfFinites(a)" * 8, "a" + " " * 1023,
)]
# a name that is both a layer and a function is the layer
EXACT += [("log + a", {"a": 0, "log": 1}), ("log .* a - abs(log)", {"a": 0, "log": 1}), ("x_1 + _y", {"x_1": 2, "_y": 0}), ("b", {"b": 1})]

# transcendentals and pow: the fp64 function narrowed once (acos in float); held at one float32 step on the host
INEXACT = [(e, NAMES) for e in (
    "-a^2", "a^2", "2^a", "a .^ b", "a .^ 2", "2 .^ a", "a.^b.^c", "a^2^3", "2^-1 * a", "abs(a) ^ 0.5", "a ^ -1",
    "exp(a)", "log(abs(a) + 0.001)", "log10(abs(a) + 0.001)", "sin(a)", "cos(a)", "tan(a)", "asin(a)", "acos(a)",
    "1.0 / log(10) * a", "exp(-square(a) / 2) / sqrt(2 * 3.14159265)", "sumOfFinites(exp(a)) + b",
)]

# (expression, names, code, a part of lio_last_error, the restatement's key)
ARG, CAPACITY = -1, -3
REFUSED = [(e, NAMES, code, part, key) for e, code, part, key in (
    ("[1, 2; 3, 4] .* a", ARG, "matrix literal", "matrix literal"),
    ("sumOfFinites([0,1,0;1,-4,1;0,1,0].*a)", ARG, "matrix literal", "matrix literal"),
    ("a + 1:3", ARG, "range", "range"),
    ("a(1, 2)", ARG, "index group", "index group"),
    ("a(0:1,:)", ARG, "index group", "index group"),
    ("(a + b)(1)", ARG, "index group", "index group"),
    ("2(1)", ARG, "index group", "index group"),
    ("a = b", ARG, "assignment", "assignment"),
    ("c = a + b", ARG, "assignment", "assignment"),
    ("a * b", ARG, "between two matrices", "two matrices"),
    ("a / b", ARG, "between two matrices", "two matrices"),
    ("a ^ b", ARG, "between two matrices", "two matrices"),
    ("a .* -b * c", ARG, "between two matrices", "two matrices"),
    ("trace(a)", ARG, "'trace'", "matrix function"), ("norm(a)", ARG, "'norm'", "matrix function"), ("size(a, 0)", ARG, "'size'", "matrix function"),
    ("transpose(a)", ARG, "'transpose'", "matrix function"), ("conjugate(a)", ARG, "'conjugate'", "matrix function"),
    ("adjoint(a)", ARG, "'adjoint'", "matrix function"), ("zeros(3)", ARG, "'zeros'", "matrix function"), ("ones(2, 2)", ARG, "'ones'", "matrix function"),
    ("eye(3)", ARG, "'eye'", "matrix function"), ("prod(a)", ARG, "'prod'", "matrix function"),
    ("sum(a) + a", ARG, "'sum'", "packet reduction"), ("mean(a)", ARG, "'mean'", "packet reduction"), ("min(a, 0)", ARG, "'min'", "packet reduction"),
    ("max(a)", ARG, "'max'", "packet reduction"), ("absmax(a, 1)", ARG, "'absmax'", "packet reduction"),
    ("sumOfFinites(a, 0) + a", ARG, "dimension", "dimension argument"), ("minOfFinites(a, 1)", ARG, "dimension", "dimension argument"),
    ("abs(a, b)", ARG, "dimension", "dimension argument"),
    ("cwiseMin(a)", ARG, "two arguments", "arguments"), ("cwiseMax(a, b, c)", ARG, "3 arguments", "arguments"),
    ("cwiseMin(2, a)", ARG, "scalar against a matrix", "dimensions"),
    ("a + d", ARG, "unknown name 'd'", "unknown name"), ("a b", ARG, "unknown name 'a b'", "unknown name"), ("elevation", ARG, "unknown name", "unknown name"),
    ("a + 1e999", ARG, "unknown name '1e999'", "unknown name"), ("a + 0x10", ARG, "unknown name '0x10'", "unknown name"),
    ("a + nan", ARG, "unknown name 'nan'", "unknown name"),
    ("sqrt", ARG, "without '('", "function without ("), ("a + abs", ARG, "without '('", "function without ("), ("sqrt a", ARG, "unknown name", "unknown name"),
    ("(a + b", ARG, "missing closing bracket", "missing bracket"), ("abs(a", ARG, "missing closing bracket", "missing bracket"),
    ("cwiseMin(a, (b)", ARG, "missing closing bracket", "missing bracket"),
    ("", ARG, "empty expression", "empty"), ("   ", ARG, "empty expression", "empty"), ("abs()", ARG, "empty expression", "empty"), ("()", ARG, "empty expression", "empty"),
    ("+a", ARG, "does not reduce", "does not reduce"), ("+ a + b", ARG, "does not reduce", "does not reduce"), ("--a", ARG, "does not reduce", "does not reduce"),
    ("a +", ARG, "does not reduce", "does not reduce"), ("a + b)", ARG, "does not reduce", "does not reduce"), ("a (", ARG, "index group", "index group"),
    ("a * * b", ARG, "lacks an operand", "operand"), ("a (b)", ARG, "index group", "index group"), ("(a) b", ARG, "without an operator", "no operator"),
    ("3", ARG, "yields a scalar", "scalar result"), ("1 + 2 * 3", ARG, "yields a scalar", "scalar result"), ("meanOfFinites(a)", ARG, "yields a scalar", "scalar result"),
    ("sqrt(sumOfFinites(square(a - meanOfFinites(a))) ./ numberOfFinites(a))", ARG, "yields a scalar", "scalar result"),
    ("a" + " " * 1024, CAPACITY, "1024 bytes", "capacity"),
    ("a" + " + a" * 64, CAPACITY, "128 ops", "capacity"),
    (chain(17), CAPACITY, "deeper than 16", "capacity"),
    ("a" + " - meanOfFinites(a)" * 9, CAPACITY, "8 map-wide reductions", "capacity"),
)]
# a leading '-' before a sum of 17 would still fit: the limit is the stack, not the text
BAD_NAMES = [({"": 0}, "a name must be"), ({"1a": 0}, "a name must be"), ({"a-b": 0}, "a name must be"), ({"a b": 0}, "a name must be"),
             ({"a": 16}, "outside 0 .. 15"), ({"a": -1}, "outside 0 .. 15")]


def layers(rows, cols, n=3, seed=0):
    """[n, rows, cols] float32 with NaN, +-inf, +-0 and denormals among ordinary values (some of them negative)"""
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    out = rng.uniform(-2.0, 2.0, (n, rows, cols)).astype(f32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-42, 1.0, -1.0, 3.0e38, 1.1754944e-38], f32)
    pick = rng.random((n, rows, cols)) < 0.3
    out[pick] = rng.choice(special, int(pick.sum()))
    return out


def unit_layers(rows, cols, n=3, seed=0):
    """finite layers for the transcendentals: inside (-1, 1) with the ends, zeros and denormals"""
    rng = np.random.default_rng(seed + 7 * rows + cols)
    out = rng.uniform(-1.0, 1.0, (n, rows, cols)).astype(f32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 1e-40, 0.5, -0.5, 0.99999994], f32)
    pick = rng.random((n, rows, cols)) < 0.2
    out[pick] = rng.choice(special, int(pick.sum()))
    return out


def with_literal_s(expression):
    return re.sub(r"\bs\b", S_LITERAL, expression)


def _wide(fn, *xs):
    with np.errstate(all="ignore"):
        return fn(*[np.asarray(x, np.float64) for x in xs]).astype(f32)


# EigenLab's self-test, the right-hand sides it compares with (EigenLab.h:1742-1925, 2064-2118), in numpy float32; pow and the
# transcendentals by the library's stated rule
S = f32(float(S_LITERAL))
SELF_TEST = {
    "a + b": lambda a, b: a + b, "a + s": lambda a, b: a + S, "s + b": lambda a, b: b + S,
    "a .+ b": lambda a, b: a + b, "a .+ s": lambda a, b: a + S, "s .+ b": lambda a, b: b + S,
    "a - b": lambda a, b: a - b, "a - s": lambda a, b: a - S, "s - b": lambda a, b: (-b) + S,
    "a .- b": lambda a, b: a - b, "a .- s": lambda a, b: a - S, "s .- b": lambda a, b: (-b) + S,
    "-a": lambda a, b: -a,
    "a .* b": lambda a, b: a * b, "a * s": lambda a, b: a * S, "s * b": lambda a, b: b * S, "a .* s": lambda a, b: a * S, "s .* b": lambda a, b: b * S,
    "a ./ b": lambda a, b: a / b, "a / s": lambda a, b: a / S, "s / b": lambda a, b: S / b, "a ./ s": lambda a, b: a / S, "s ./ b": lambda a, b: S / b,
    "abs(a) .^ b": lambda a, b: _wide(np.power, np.abs(a), b), "abs(a) ^ s": lambda a, b: _wide(np.power, np.abs(a), S),
    "s ^ b": lambda a, b: _wide(np.power, S, b), "abs(a) .^ s": lambda a, b: _wide(np.power, np.abs(a), S), "s .^ b": lambda a, b: _wide(np.power, S, b),
    "abs(a)": lambda a, b: np.abs(a), "sqrt(abs(a))": lambda a, b: np.sqrt(np.abs(a)),
    "exp(abs(a) + 0.001)": lambda a, b: _wide(np.exp, np.abs(a) + f32(0.001)), "log(abs(a) + 0.001)": lambda a, b: _wide(np.log, np.abs(a) + f32(0.001)),
    "log10(abs(a) + 0.001)": lambda a, b: _wide(np.log, np.abs(a) + f32(0.001)) * f32(1.0 / math.log(10)),
    "sin(a)": lambda a, b: _wide(np.sin, a), "cos(a)": lambda a, b: _wide(np.cos, a), "tan(a)": lambda a, b: _wide(np.tan, a),
    "asin(a)": lambda a, b: _wide(np.arcsin, a), "acos(a)": lambda a, b: _wide(np.arccos, a),
    "cwiseMin(a, b)": lambda a, b: np.minimum(a, b), "cwiseMax(a, b)": lambda a, b: np.maximum(a, b),
}
SELF_TEST_EXACT = {e for e in SELF_TEST if not re.search(r"\^|exp|log|sin|cos|tan", e)}
