"""The Python binding against include/liogpu.h, without a GPU: every prototype against its line of api.CAPI, every field of
every struct against its ctypes mirror (gcc's sizeof / offsetof), the load-time binding over a library that lacks a symbol,
the config helpers and the close() / __del__ base class."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every ctypes.Structure of api.py -> the C struct it mirrors; a new struct takes one line here
STRUCTS = {
    "S2MConfig": "lio_s2m_config", "S2MResult": "lio_s2m_result", "S2MProfile": "lio_s2m_profile",
    "DebugGnRecord": "lio_debug_gn_record", "GridPlanInfo": "lio_grid_plan_info",
    "DeskewConfig": "lio_deskew_config", "PC2Layout": "lio_pc2_layout", "RangeImageConfig": "lio_range_image_config",
    "FeatureConfig": "lio_feature_config", "NearbyConfig": "lio_nearby_config",
    "IcpConfig": "lio_icp_config", "IcpResult": "lio_icp_result", "IcpClouds": "lio_icp_clouds", "IcpGridInfo": "lio_icp_grid_info",
    "ScConfig": "lio_sc_config", "ScResult": "lio_sc_result",
    "LocalMapConfig": "lio_local_map_config", "LocalMapInfo": "lio_local_map_info",
    "HeightMapConfig": "lio_height_map_config", "HeightMapInfo": "lio_height_map_info",
    "TerrainConfig": "lio_terrain_config", "TerrainInfo": "lio_terrain_info",
    "GlobalMapConfig": "lio_global_map_config", "GlobalMapInfo": "lio_global_map_info", "ExportConfig": "lio_export_config",
    "OgmConfig": "lio_ogm_config", "OgmInfo": "lio_ogm_info", "SdfConfig": "lio_sdf_config", "SdfInfo": "lio_sdf_info",
    "MedianFillConfig": "lio_median_fill_config", "MedianFillInfo": "lio_median_fill_info",
    "PlanningMapBuffers": "lio_planning_map_buffers",
    "GridSampleConfig": "lio_grid_sample_config", "GridSampleInfo": "lio_grid_sample_info", "GridInfo": "lio_grid_desc",
    "GridRegion": "lio_grid_region", "GridRegionConfig": "lio_grid_region_config", "GridRegionStat": "lio_grid_region_stat",
    "GridRegionInfo": "lio_grid_region_info",
}
SCALARS = {"int32_t": C.c_int32, "int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
           "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int64_t": C.c_int64}
RETURNS = {"int": C.c_int, "void": None, "size_t": C.c_size_t, "float": C.c_float, "void *": C.c_void_p, "const char *": C.c_char_p}


@pytest.fixture(scope="module")
def api(pkg):
    return importlib.import_module("lio-slam_amd.api")


@pytest.fixture(scope="module")
def header():
    """include/liogpu.h without its comments"""
    src = open(os.path.join(ROOT, "include", "liogpu.h")).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", src, flags=re.S))


def _squeeze(s):
    return re.sub(r"\s*\*\s*", " * ", " ".join(s.split())).replace("* *", "**").strip()


def _is_pointer_kind(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_every_prototype_matches_its_binding(api, header):
    structs = {getattr(api, py): c for py, c in STRUCTS.items()}
    protos = re.findall(r"([A-Za-z_][\w \t\*]*?)\b(lio_\w+)\s*\(([^()]*)\)\s*;", header)
    names = [name for _, name, _ in protos]
    assert len(set(names)) == len(names)
    assert set(names) == set(api.CAPI), set(names) ^ set(api.CAPI)
    n_params = 0
    for ret, name, params in protos:
        restype, argtypes = api.CAPI[name]
        ret = _squeeze(ret)
        assert ret in RETURNS, f"{name}: return type '{ret}' is not one this test knows"
        assert restype is RETURNS[ret], f"{name}: returns '{ret}', bound as {restype}"
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        assert len(params) == len(argtypes), f"{name}: {len(params)} parameters, {len(argtypes)} argtypes"
        for k, (p, t) in enumerate(zip(params, argtypes)):
            what = f"{name} parameter {k} '{p}', bound as {t}"
            n_params += 1
            if "*" in p or "[" in p:
                assert _is_pointer_kind(t), what
                pointee = getattr(t, "_type_", None) if t not in (C.c_void_p, C.c_char_p) else None
                base = re.match(r"(?:const\s+)?(\w+)", p).group(1)
                if isinstance(pointee, type) and issubclass(pointee, C.Structure):
                    assert base == structs[pointee], what
                elif pointee is not None and base in SCALARS:          # POINTER(c_float) for a `const float *`, not for a double's
                    assert pointee is SCALARS[base], what
                continue
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s+\w+", p)
            assert m and m.group(1) in SCALARS, f"{what}: a scalar spelling this test does not know"
            assert t is SCALARS[m.group(1)], what
    print(f"{len(protos)} prototypes, {n_params} parameters compared")
    assert len(protos) == len(api.CAPI) == len(api.EXPORTS)


def test_every_struct_field_matches_c(api, header):
    mirrors = {name for name, v in vars(api).items() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == api.__name__}
    assert mirrors == set(STRUCTS), mirrors ^ set(STRUCTS)
    bodies = dict((c, body) for body, c in re.findall(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(lio_\w+)\s*;", header, flags=re.S))
    assert set(bodies) == set(re.findall(r"\}\s*(lio_\w+)\s*;", header)) == set(STRUCTS.values()), set(bodies) ^ set(STRUCTS.values())
    assert len(set(STRUCTS.values())) == len(STRUCTS)
    lines, expect = [], []
    for py, c in STRUCTS.items():
        cls = getattr(api, py)
        fields = [f[0] for f in cls._fields_]
        declared = [n for stmt in bodies[c].split(";") for n in re.findall(r"(\w+)\s*(?:\[[^\]]*\]\s*)*(?:,|$)", stmt.strip())]
        assert fields == declared, (py, c, fields, declared)
        lines.append(f'printf("%zu\\n", sizeof({c}));')
        expect.append((f"sizeof({c})", C.sizeof(cls)))
        for f in fields:
            lines.append(f'printf("%zu %zu\\n", offsetof({c}, {f}), sizeof((({c} *)0)->{f}));')
            expect.append((f"offsetof({c}, {f})", getattr(cls, f).offset))
            expect.append((f"sizeof({c}.{f})", getattr(cls, f).size))
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"liogpu.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c_file, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c_file, "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c_file, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert len(got) == len(expect)
    wrong = [(what, c_val, py_val) for (what, py_val), c_val in zip(expect, got) if c_val != py_val]
    assert not wrong, wrong
    n_fields = sum(len(getattr(api, py)._fields_) for py in STRUCTS)
    print(f"{len(STRUCTS)} structs: {len(STRUCTS) + n_fields} sizes and offsets, {n_fields} field sizes compared")


def test_missing_symbol_is_skipped_at_load_and_fails_at_call(api):
    class Fn:
        pass

    class OlderBuild:
        """every symbol of the table but one"""
        def __getattr__(self, name):
            if name == "lio_s2m_launch_forms" or name not in api.CAPI:
                raise AttributeError(name)
            fn = self.__dict__[name] = Fn()
            return fn

    lib = OlderBuild()
    assert api._bind(lib) is lib
    assert set(vars(lib)) == set(api.CAPI) - {"lio_s2m_launch_forms"}
    for name, fn in vars(lib).items():
        assert (fn.restype, fn.argtypes) == api.CAPI[name], name
    assert lib.lio_kf_store_points.restype is C.c_size_t and lib.lio_s2m_destroy.restype is None
    with pytest.raises(AttributeError):
        lib.lio_s2m_launch_forms


CONFIGS = {"deskew": "DeskewConfig", "nearby": "NearbyConfig", "icp": "IcpConfig", "sc": "ScConfig", "local_map": "LocalMapConfig",
           "global_map": "GlobalMapConfig", "height_map": "HeightMapConfig", "terrain": "TerrainConfig", "ogm": "OgmConfig", "sdf": "SdfConfig",
           "median_fill": "MedianFillConfig", "grid_sample": "GridSampleConfig", "grid_region": "GridRegionConfig"}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_default_config_returns_its_struct_and_refuses_a_stray_key(api, name):
    make = getattr(api, name + "_default_config")
    cfg = make()
    assert type(cfg) is getattr(api, CONFIGS[name])
    first = cfg._fields_[0][0]
    if not isinstance(getattr(cfg, first), C.Array):
        assert getattr(make(**{first: 1}), first) == 1
    with pytest.raises(AttributeError, match="nonsense"):
        make(nonsense=1)


def test_config_conversions(api):
    assert len([n for n in vars(api) if n.endswith("_default_config") and not n.startswith("_")]) == len(CONFIGS)
    assert list(api.height_map_default_config(voxel=(0.5, 0.25, 2.0)).voxel) == [0.5, 0.25, 2.0]
    cfg = api.s2m_config(device_ids=[2, 3], max_iters=7)
    assert type(cfg) is api.S2MConfig and list(cfg.device_ids)[:2] == [2, 3] and cfg.max_iters == 7
    base = api.s2m_config()
    assert list(cfg.device_ids)[2:] == list(base.device_ids)[2:] and base.max_iters == 30
    with pytest.raises(AttributeError, match="nonsense"):
        api.s2m_config(nonsense=1)


def test_owner_releases_once_and_never_before_the_resource_exists(api):
    class Owned(api._Owner):
        released = 0

        def __init__(self, fail=False):
            if fail:
                raise RuntimeError("before the handle")
            self.h = C.c_void_p(1234)

        def _release(self):
            assert self.h.value == 1234                      # the resource is still there while it is released
            type(self).released += 1

    o = Owned()
    o.close()
    assert Owned.released == 1 and isinstance(o.h, C.c_void_p) and not o.h
    o.close()
    o.__del__()
    assert Owned.released == 1
    failed = Owned.__new__(Owned)
    with pytest.raises(RuntimeError):
        failed.__init__(fail=True)
    failed.close()
    failed.__del__()
    assert Owned.released == 1

    class Address(api._Owner):
        _owned, released = "ptr", 0

        def _release(self):
            type(self).released += 1
            raise RuntimeError("a release that fails")

    a = Address()
    a.ptr = 4096
    a.__del__()                                              # swallowed
    assert Address.released == 1
    with pytest.raises(RuntimeError):
        a.close()
    for cls in (api.ScanToMap, api.KeyframeStore, api.Sdf, api.Grid, api.DeviceBuffer, api.PinnedBuffer):
        assert issubclass(cls, api._Owner) and "close" not in vars(cls) and "__del__" not in vars(cls)
        assert cls._owned == ("ptr" if cls in (api.DeviceBuffer, api.PinnedBuffer) else "h")
        cls.__new__(cls).close()                             # an object whose __init__ never ran
