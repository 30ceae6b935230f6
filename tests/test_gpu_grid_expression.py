"""lio_grid_filter_expression on the device through the Python wrapper against the numpy restatement of EigenLab's passes
(tests/grid_expression_restate.py, which tests/test_grid_expression_cpu.py holds the host route to) on the case lists of
tests/grid_expression_cases.py.  Exact operations: word for word where the value is not a NaN, the NaN masks equal (a NaN's
sign and payload are the platform's); tolerance 0.  Transcendentals and pow: against float32(numpy fp64 function(float64(x)))
of the device's own input layer -- acos at the project's ACOS_ULPS = 2 (tests/test_gpu_terrain.py), the fp64-routed ones at
1 float32 step (derived: two doubles that differ by far less than a float32 step round, monotonically, to the same or adjacent
floats), log10 bit for bit as the device's own log layer times the constant.  Three cross-checks against texts merged before
this one, bit for bit: the terrain layers' slope, roughness and traversability, the window filter's STDDEV, the duplication.
Parity with grid_map, EigenLab and Eigen themselves is unpinned (none can be built here)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_expression_cases as K                              # noqa: E402
import grid_expression_restate as R                            # noqa: E402
import terrain_restate as T                                    # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
CHUNK = 1024                                                   # LIO_GX_CHUNK of csrc/lio_gridexpr.h: the walker's cells between two folds
LANES = 256                                                    # LIO_GX_LANES: k_gx_eval's block
ACOS_ULPS = 2                                                  # tests/test_gpu_terrain.py:28-30
# 1 x 1; a row; a column; two blocks, the last one partial; more than two of the walker's chunks and no multiple of one
SHAPES = ((1, 1), (1, 7), (7, 1), (33, 9), (37, 59))
assert LANES < 33 * 9 < 2 * LANES and 37 * 59 > 2 * CHUNK and 37 * 59 % CHUNK


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def upload(g, layers, res=0.25, pos=(3.0, -2.0)):
    rows, cols = layers[0].shape
    g.set_layers(np.stack(layers), res, (rows * res, cols * res), pos)


@functools.lru_cache(maxsize=None)
def restated(expression, names, shape):
    """the restatement's layer for a case on K.layers(shape), computed once"""
    layers = K.layers(*shape)
    out, exact, p = R.evaluate(expression, {k: layers[i] for k, i in names})
    out.setflags(write=False)
    return out, exact, p.n_passes, p.stack_depth


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_cases_word_for_word(pkg, shape):
    layers = K.layers(*shape)
    g = pkg.Grid()
    upload(g, list(layers))
    for expression, names in K.EXACT:
        want, exact, n_passes, depth = restated(expression, tuple(names.items()), shape)
        assert exact
        info = g.filter_expression(expression, names, 3)
        got = g.layer(3)
        assert R.same_words(got, want), (expression, shape)
        assert (info["rows"], info["cols"], info["n_passes"], info["stack_depth"]) == (shape[0], shape[1], n_passes, depth), expression
        assert info["n_finite"] == np.isfinite(want).sum(), expression
    for k in range(3):                                         # the inputs are only read
        assert np.array_equal(bits(g.layer(k)), bits(layers[k]))
    g.close()


@pytest.mark.parametrize("shape", ((7, 1), (37, 59)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_reduction_whose_first_coefficients_are_nan_then_inf(pkg, shape):
    z = K.layers(*shape)[0].copy()
    flat = z.reshape(-1, order="F")
    flat[0], flat[1] = np.nan, np.inf
    z = flat.reshape(shape, order="F")
    assert np.isnan(z[0, 0]) and (z[1, 0] if shape[0] > 1 else z[0, 1]) == np.inf
    one = np.ones(shape, f32)
    g = pkg.Grid()
    upload(g, [z, one])
    for name in R.REDUCTIONS:
        for argument in ("a", "-a", "square(a)"):
            e = f"{name}({argument}) * one"
            want, exact, _ = R.evaluate(e, {"a": z, "one": one})
            g.filter_expression(e, {"a": 0, "one": 1}, 2)
            assert exact and R.same_words(g.layer(2), want), (e, g.layer(2)[0, 0], want[0, 0])
    g.close()


def test_out_layer_read_new_and_a_failing_call(pkg):
    shape = (33, 9)
    layers = K.layers(*shape)
    g = pkg.Grid()
    upload(g, list(layers))
    e = "a - meanOfFinites(a) + b"
    want, _, _ = R.evaluate(e, {"a": layers[0], "b": layers[1]})
    g.filter_expression(e, {"a": 0, "b": 1}, 0)               # out_layer is a layer the expression reads: from the old values
    assert R.same_words(g.layer(0), want)
    assert np.array_equal(bits(g.layer(1)), bits(layers[1])) and g.info().layer_mask == 0b111
    g.filter_expression("cwiseMax(b, c)", {"b": 1, "c": 2, "unused": 9}, 12)     # a new layer; a listed layer the object lacks is not read
    assert g.info().layer_mask == 0b111 | 1 << 12
    assert R.same_words(g.layer(12), np.where(layers[1] < layers[2], layers[2], layers[1]))
    held = [g.layer(k) for k in (0, 1, 2, 12)]
    with pytest.raises(pkg.LioError, match="reads a layer the object does not hold"):
        g.filter_expression("b + absent", {"b": 1, "absent": 9}, 7)
    with pytest.raises(pkg.LioError, match="128 ops"):
        g.filter_expression("b" + " + b" * 64, {"b": 1}, 7)
    with pytest.raises(pkg.LioError, match="outside 0 .. 15"):
        g.filter_expression("b", {"b": 1}, 16)
    assert g.info().layer_mask == 0b111 | 1 << 12              # a failing call leaves the layer set as it was
    for k, was in zip((0, 1, 2, 12), held):
        assert np.array_equal(bits(g.layer(k)), bits(was))
    g.close()
    empty = pkg.Grid()
    with pytest.raises(pkg.LioError, match="holds no layers"):
        empty.filter_expression("a", {"a": 0}, 1)
    empty.close()


def test_transcendentals_and_pow(pkg):
    shape = (33, 9)
    rng = np.random.default_rng(11)
    unit = K.unit_layers(*shape)[0]
    wide = rng.uniform(-50.0, 50.0, shape).astype(f32)
    small = rng.uniform(-3.0, 3.0, shape).astype(f32)
    g = pkg.Grid()
    upload(g, [unit, wide, small])
    u, w, s = (g.layer(k) for k in range(3))                   # the device's own input layers
    names = {"u": 0, "w": 1, "s": 2}

    def wide_fn(fn, *xs):
        with np.errstate(all="ignore"):
            return fn(*[np.asarray(x, np.float64) for x in xs]).astype(f32)
    cases = (("exp(w)", wide_fn(np.exp, w), 1), ("exp(u)", wide_fn(np.exp, u), 1), ("log(abs(w))", wide_fn(np.log, np.abs(w)), 1), ("log(u)", wide_fn(np.log, u), 1),
             ("sin(w)", wide_fn(np.sin, w), 1), ("sin(u)", wide_fn(np.sin, u), 1), ("cos(w)", wide_fn(np.cos, w), 1), ("cos(u)", wide_fn(np.cos, u), 1),
             ("tan(w)", wide_fn(np.tan, w), 1), ("tan(u)", wide_fn(np.tan, u), 1), ("asin(u)", wide_fn(np.arcsin, u), 1), ("asin(s)", wide_fn(np.arcsin, s), 1),
             ("acos(u)", wide_fn(np.arccos, u), ACOS_ULPS), ("acos(s)", wide_fn(np.arccos, s), ACOS_ULPS),
             ("abs(w) .^ s", wide_fn(np.power, np.abs(w), s), 1), ("w .^ s", wide_fn(np.power, w, s), 1), ("w ^ 2", wide_fn(np.power, w, 2.0), 1),
             ("2 ^ s", wide_fn(np.power, 2.0, s), 1), ("abs(w) ^ 0.5", wide_fn(np.power, np.abs(w), 0.5), 1), ("s ^ -1", wide_fn(np.power, s, -1.0), 1),
             ("u ^ 3", wide_fn(np.power, u, 3.0), 1))
    for e, want, bar in cases:
        g.filter_expression(e, names, 3)
        worst, n = R.ulps(g.layer(3), want)
        print(f"  {e}: largest distance {worst} float32 steps, {n} of {want.size} cells not identical (bar {bar})")
        assert worst <= bar, (e, worst, n)
    for arg, x in (("abs(w)", np.abs(w)), ("u", u)):           # log10 is the device's own log times the constant, a float product
        g.filter_expression(f"log({arg})", names, 3)
        g.filter_expression(f"log10({arg})", names, 4)
        with np.errstate(all="ignore"):
            assert R.same_words(g.layer(4), g.layer(3) * R.INV_LN10), arg
    g.close()


def test_against_the_terrain_layers(pkg):
    """scene A of tests/test_gpu_terrain.py by its recipe: the three expressions of the demo filter chain and the two
    thresholds reproduce the layers lio_terr_cell hard-wires, from the device's own normals and smooth layer"""
    chain = [e["expression"] for e in K.GOLDEN["yaml"]]
    pos = (60.0, -35.0)
    grid = T.scene_a(pos)
    rows, cols = grid.shape
    cfg = pkg.terrain_default_config(normal_radius=0.3, smooth_radius=0.6, edge_window_length=0.75)
    assert (cfg.slope_weight, cfg.slope_critical, cfg.roughness_weight, cfg.roughness_critical) == (0.5, f32(0.6), 0.5, f32(0.1))
    d, _ = pkg.terrain_layers(grid, 0.25, (rows * 0.25, cols * 0.25), pos, cfg)
    g = pkg.Grid()
    upload(g, [grid, d["smooth"], d["normal_z"]], 0.25, pos)
    g.filter_expression(chain[0], {"normal_vectors_z": 2}, 3)
    g.filter_expression(chain[1], {"elevation_inpainted": 0, "elevation_smooth": 1}, 4)
    g.filter_expression(chain[2], {"slope": 3, "roughness": 4}, 5)
    g.filter_threshold(5, 5, False, 0.0, 0.0)
    g.filter_threshold(5, 5, True, 1.0, 1.0)
    for k, name in ((3, "slope"), (4, "roughness"), (5, "traversability")):
        assert R.same_words(g.layer(k), d[name]), name
    assert np.isfinite(d["traversability"]).any() and (d["slope"] > 0).any()
    g.close()


def test_against_the_window_filter_and_the_duplication(pkg):
    rng = np.random.default_rng(3)
    x = rng.uniform(-2.0, 2.0, (9, 9)).astype(f32)
    x[0, 0], x[8, 3], x[2, 7], x[5, 5] = np.nan, np.inf, np.nan, -np.inf
    g = pkg.Grid()
    upload(g, [x])
    e = K.GOLDEN["yaml_scalar"][1]["expression"].replace("slope", "x")
    g.filter_expression("0 * x + " + e, {"x": 0}, 1)           # the scalar as a layer: at a finite cell 0 * x + s is s
    g.filter_window(0, 2, pkg.GW_STDDEV, pkg.GW_EMPTY, 9)       # the centre's 9 x 9 window is the map
    a, b = g.layer(1)[4, 4], g.layer(2)[4, 4]
    assert np.isfinite(a) and bits(a) == bits(b), (a, b)
    z = K.layers(33, 9)[0]
    upload(g, [z])
    g.filter_expression("x", {"x": 0}, 1)
    g.duplicate_layer(0, 2)
    assert np.array_equal(bits(g.layer(1)), bits(g.layer(2))) and np.array_equal(bits(g.layer(1)), bits(z))
    g.close()


def test_kernel_time_hook(pkg):
    lib = pkg.load_library()
    g = pkg.Grid()
    upload(g, list(K.layers(37, 59)))
    ms = (C.c_float * 2)(-1.0, -1.0)
    assert lib.lio_grid_expression_debug_kernel_ms(1, None) == 0
    g.filter_expression("a - meanOfFinites(a)", K.NAMES, 3)
    assert lib.lio_grid_expression_debug_kernel_ms(0, ms) == 0 and ms[0] > 0.0 and ms[1] > 0.0
    g.filter_expression("a + b", K.NAMES, 3)
    assert lib.lio_grid_expression_debug_kernel_ms(0, ms) == 0 and list(ms) == [0.0, 0.0]      # off again
    g.close()
