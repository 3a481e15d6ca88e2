"""The ctypes prototypes and struct mirrors of loltracer_amd/gpu.py and scene.py against the text of the four headers: every
function's return type, parameter count and parameter types, every mirrored struct's field names, order and types (no GPU).

The comparison is a pure function of (header text, table): `function_findings` and `struct_findings` return a list of sentences,
each beginning with the function or struct it is about, and the tests at the bottom feed them doctored header text to see them bite."""
import ctypes as C
import os
import re
import types

from loltracer_amd import gpu, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.POINTER

TABLES = {"lol_gpu.h": gpu._LOL_GPU_H, "lol_gpu_diag.h": gpu._LOL_GPU_DIAG_H, "lol_gpu_testing.h": gpu._LOL_GPU_TESTING_H,
          "lol_scene.h": S._LOL_SCENE_H}

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long": C.c_long, "unsigned short": C.c_ushort,
           "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "uint8_t": C.c_uint8, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
OPAQUE = ("void", "lol_gpu", "lol_gpu_multi")                # T* -> c_void_p, T** -> POINTER(c_void_p)
MIRRORS = {                                                   # every struct of the headers that Python mirrors, by name
    "lol_v3": S.V3, "lol_material": S.Material, "lol_light": S.Light, "lol_camera": S.Camera, "lol_node": S.Node,
    "lol_scene": S.SceneStruct, "lol_op": S.Op, "lol_program": S.Program, "lol_frame_camera": S.FrameCamera,
    "lol_gpu_rows": gpu.Rows, "lol_gpu_pixel_format": gpu.PixelFormat, "lol_gpu_tile_order_info": gpu.TileOrderInfo,
    "lol_gpu_debug": gpu.Debug, "lol_gpu_hits": gpu.Hits, "lol_gpu_hit": gpu.Hit, "lol_gpu_shades": gpu.Shades,
    "lol_gpu_light_factor": gpu.LightFactor, "lol_gpu_light_passes": gpu.LightPasses, "lol_gpu_relit": gpu.Relit,
    "lol_gpu_shade_math_info": gpu.ShadeMathInfo, "lol_gpu_testing_schedule_info": gpu._ScheduleInfo,
}

# Where the mirror deliberately says something else than the header, by (function, parameter): the type the mirror has.  A list, not
# a rule: a rule would excuse the next mismatch.  An entry that no longer applies is a finding too.
_DEVICE_LISTS = {                                             # lists in device memory: callers pass integer addresses
    "rays_dev": ("lol_gpu_trace_rays", "lol_gpu_shade_rays", "lol_gpu_light_rays", "lol_gpu_light_update_rays",
                 "lol_gpu_trace_scene_rays", "lol_gpu_shade_scene_rays"),
    "xy_dev": ("lol_gpu_trace_pixels", "lol_gpu_shade_pixels", "lol_gpu_light_pixels", "lol_gpu_light_update_pixels",
               "lol_gpu_trace_scene_pixels", "lol_gpu_shade_scene_pixels"),
}
LATITUDES = {(fn, param): C.c_void_p for param, fns in _DEVICE_LISTS.items() for fn in fns}
LATITUDES.update({("lol_gpu_powf_batch", p): C.c_void_p for p in ("x_dev", "y_dev", "out_dev")})
LATITUDES.update({("lol_gpu_sdf_batch", p): C.c_void_p for p in ("pts_dev", "dist_dev", "id_dev")})
LATITUDES.update({("lol_gpu_code_key", "code"): C.c_char_p,                           # const void* byte buffers taken as bytes
                  ("lol_gpu_testing_has_return_clobbering_branch", "code"): C.c_char_p})


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _code(text):
    """the header without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M)


def _declarator(text):
    """'const  lol_program *look' -> ('const lol_program*', 'look', []); 'float out[3][4]' -> ('float', 'out', [3, 4])"""
    m = re.match(r"(.*?)(\w+)((?:\s*\[\s*\d+\s*\])*)$", text.strip(), flags=re.S)
    base = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
    return base, m.group(2), [int(d) for d in re.findall(r"\d+", m.group(3))]


def parse_functions(text):
    """{name: (return type, [(type, name, array dims)])} of every function the header declares"""
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", _code(text), flags=re.S)
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(\w+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(3).strip()
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        out[m.group(2)] = (ret, [] if params in ("", "void") else [_declarator(p) for p in params.split(",")])
    return out


def parse_structs(text):
    """{name: [(type, field, array dims)]} of every `typedef struct name { ... } name;`; `uint32_t id, steps;` declares two fields"""
    out = {}
    for m in re.finditer(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", _code(text), flags=re.S):
        fields = []
        for stmt in m.group(2).split(";"):
            if stmt.strip():
                first, *rest = stmt.split(",")
                base, name, dims = _declarator(first)
                fields.append((base, name, dims))
                fields += [(base,) + _declarator(r)[1:] for r in rest]
        out[m.group(1)] = fields
    return out


def c_type(ctype, dims=(), device_pointers=False):
    """The ctypes type of a C type as the headers write it.  device_pointers: a pointer is c_void_p whatever it points to (the fields
    of the lol_gpu structs, which hold device addresses)."""
    t = re.sub(r"\bconst\b", "", ctype).strip()
    base, stars = t.rstrip("*").strip(), len(t) - len(t.rstrip("*"))
    if stars and device_pointers:
        el = C.c_void_p
    elif base == "char" and stars == 1:
        el = C.c_char_p
    elif base in OPAQUE and stars in (1, 2):
        el = C.c_void_p if stars == 1 else P(C.c_void_p)
    else:
        el = SCALARS[base] if base in SCALARS else MIRRORS[base]          # KeyError: a type this mapping does not know
        for _ in range(stars):
            el = P(el)
    for d in reversed(dims):
        el = el * d
    return el


def param_type(ctype, dims):
    """a parameter's ctypes type: an array parameter is a pointer to its element (float ms[3] is float*, float out[3][4] is
    float (*)[4], char out[17] is char*)"""
    if not dims:
        return c_type(ctype)
    if not dims[1:]:
        return c_type(ctype + "*")
    return P(c_type(ctype, dims[1:]))


def function_findings(text, table, latitudes):
    """What differs between the header's declarations and the table, both ways; [] when they agree."""
    declared, out = parse_functions(text), []
    out += [f"{n}: declared in the header, not in the table" for n in declared if n not in table]
    out += [f"{n}: in the table, not declared in the header" for n in table if n not in declared]
    used = set()
    for name, (ret, params) in declared.items():
        if name not in table:
            continue
        restype, argtypes = table[name]
        try:
            if restype is not (None if ret == "void" else c_type(ret)):
                out.append(f"{name}: returns {ret}, the table says {restype}")
            if len(argtypes) != len(params):
                out.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
                continue
            for (ctype, pname, dims), have in zip(params, argtypes):
                want = param_type(ctype, dims)
                if (name, pname) in latitudes and have is not want:
                    used.add((name, pname))
                    want = latitudes[name, pname]
                if have is not want:
                    out.append(f"{name}: parameter {pname} is {ctype}{''.join('[%d]' % d for d in dims)} = {want}, the table says {have}")
        except KeyError as e:
            out.append(f"{name}: no mapping for the type {e}")
    out += [f"{fn}: the latitude for {p} is not needed" for fn, p in latitudes if fn in table and (fn, p) not in used]
    return out


def struct_findings(text, mirrors, device_pointers):
    """What differs between the header's structs and their mirror classes: field names, their order, their types."""
    out = []
    for name, fields in parse_structs(text).items():
        if name not in mirrors:
            out.append(f"{name}: no mirror class named")
            continue
        have = list(mirrors[name]._fields_)
        if [f for _, f, _ in fields] != [f for f, _ in have]:
            out.append(f"{name}: fields {[f for _, f, _ in fields]}, the mirror has {[f for f, _ in have]}")
            continue
        for (ctype, field, dims), (_, t) in zip(fields, have):
            want = c_type(ctype, dims, device_pointers)
            if t is not want:
                out.append(f"{name}: field {field} is {ctype} = {want}, the mirror says {t}")
    return out


def latitudes_of(table):
    return {k: v for k, v in LATITUDES.items() if k[0] in table}


def named(findings):
    return {f.split(":")[0] for f in findings}


def test_every_prototype_is_the_headers():
    for name, table in TABLES.items():
        assert len(parse_functions(header(name))) >= 10, name                     # (the parser found the declarations at all)
        assert function_findings(header(name), table, latitudes_of(table)) == [], name
    assert {fn for fn, _ in LATITUDES} <= {fn for table in TABLES.values() for fn in table}
    assert gpu.EXPORTED_SYMBOLS == list(gpu._LOL_GPU_H) and gpu.DIAG_SYMBOLS == list(gpu._LOL_GPU_DIAG_H)
    assert gpu.TESTING_SYMBOLS == list(gpu._LOL_GPU_TESTING_H)
    assert next(iter(gpu._LOL_GPU_H)) == "lol_gpu_abi_version"


def test_every_struct_mirror_is_the_headers():
    seen = set()
    for name in TABLES:
        structs = parse_structs(header(name))
        assert struct_findings(header(name), MIRRORS, device_pointers=name != "lol_scene.h") == [], name
        seen |= set(structs)
    assert seen == set(MIRRORS)
    hit = dict((f, (t, d)) for t, f, d in parse_structs(header("lol_gpu.h"))["lol_gpu_hit"])
    assert hit == {"dist": ("float", []), "id": ("uint32_t", []), "steps": ("uint32_t", []), "normal": ("float", [3])}


def test_the_loaded_libraries_carry_the_tables():
    """what gpu_lib() and host_lib() bound is what the tables say"""
    for lib, tables in ((gpu.gpu_lib(), [t for n, t in TABLES.items() if n != "lol_scene.h"]), (S.host_lib(), [S._LOL_SCENE_H])):
        for table in tables:
            for name, (restype, argtypes) in table.items():
                fn = getattr(lib, name)
                assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_the_parser_reads_array_parameters_and_every_return_type():
    diag = parse_functions(header("lol_gpu_diag.h"))
    assert diag["lol_gpu_adaptive_pass_ms"] == ("int", [("lol_gpu*", "ctx", []), ("float", "ms", [3])])
    assert diag["lol_gpu_cull_bounds_clusters"][1][2] == ("float", "out", [3, 4]) and param_type("float", [3, 4]) is P(C.c_float * 4)
    assert diag["lol_gpu_roctx_ranges"] == ("long", []) and diag["lol_gpu_code_key"][0] == "void"
    assert parse_functions(header("lol_scene.h"))["lol_scene_new"] == ("lol_scene*", [])
    assert parse_functions(header("lol_gpu.h"))["lol_gpu_create"] == ("int", [("int", "device", []), ("lol_gpu**", "out", [])])
    assert param_type("float", [3]) is P(C.c_float) and param_type("char", [17]) is C.c_char_p
    assert c_type("const lol_frame_camera*") is P(S.FrameCamera) and c_type("lol_gpu**") is P(C.c_void_p)


def doctored(text, old, new, count=1):
    out, n = re.subn(old, new, text, count=count, flags=re.S)
    assert n == 1, old
    return out


def test_a_doctored_header_is_caught_at_the_function():
    text, table = header("lol_gpu.h"), gpu._LOL_GPU_H
    lat = latitudes_of(table)
    # size_t n of lol_gpu_trace_rays turned into int n
    bad = doctored(text, r"(\blol_gpu_trace_rays\([^)]*?)size_t(\s+n\b)", r"\1int\2")
    assert named(function_findings(bad, table, lat)) == {"lol_gpu_trace_rays"}
    # two adjacent parameters of lol_gpu_render_views swapped (the destination and its pitch)
    decl = parse_functions(text)["lol_gpu_render_views"][1]
    i = [p[1] for p in decl].index("pitch_bytes")
    assert c_type(decl[i - 1][0]) is not c_type(decl[i][0])
    bad = doctored(text, r"(\blol_gpu_render_views\([^)]*?)(\w+\*?\s+%s)(\s*,\s*)(\w+\s+pitch_bytes)" % decl[i - 1][1], r"\1\4\3\2")
    assert named(function_findings(bad, table, lat)) == {"lol_gpu_render_views"}
    # one declaration removed
    bad = doctored(text, r"\bint\s+lol_gpu_sync\([^)]*\);", "")
    assert function_findings(bad, table, lat) == ["lol_gpu_sync: in the table, not declared in the header"]
    # one invented declaration added
    bad = text.replace("int  lol_gpu_device_count(void);", "int  lol_gpu_device_count(void);\nint lol_gpu_invented(lol_gpu* ctx, float x);", 1)
    assert function_findings(bad, table, lat) == ["lol_gpu_invented: declared in the header, not in the table"]
    # two fields of lol_gpu_light_passes swapped
    bad = doctored(text, r"(uint32_t\*\s+hit_id;)([^;]*?)(float\*\s+hit_dist;)", r"\3\2\1")
    assert named(struct_findings(bad, MIRRORS, True)) == {"lol_gpu_light_passes"}
    # ... and a field of another type, a parameter less, another return type
    bad = doctored(text, r"size_t(\s+light_stride;)", r"uint32_t\1")
    assert named(struct_findings(bad, MIRRORS, True)) == {"lol_gpu_light_passes"}
    bad = doctored(text, r"(\blol_gpu_pick\([^)]*?),\s*lol_gpu_hit\*\s+\w+\)", r"\1)")
    assert named(function_findings(bad, table, lat)) == {"lol_gpu_pick"}
    bad = doctored(text, r"\bvoid(\s+lol_gpu_destroy\()", r"int\1")
    assert named(function_findings(bad, table, lat)) == {"lol_gpu_destroy"}
    # the same from the other side: the header as it is, one table entry wrong
    assert named(function_findings(text, dict(table, lol_gpu_sync=(C.c_int, [C.c_int])), lat)) == {"lol_gpu_sync"}


def test_binding_onto_a_library_that_lacks_a_symbol_binds_the_rest():
    """a library named by LOL_GPU_LIB for an A/B run may be an older build: what it lacks stays unbound, nothing raises"""
    table = gpu._LOL_GPU_DIAG_H
    lacking = "lol_gpu_shade_math"
    stub = types.SimpleNamespace(**{n: types.SimpleNamespace(restype="unset", argtypes="unset") for n in table if n != lacking})
    S._bind_prototypes(stub, table)
    assert not hasattr(stub, lacking)
    for name, (restype, argtypes) in table.items():
        if name != lacking:
            assert getattr(stub, name).restype is restype and getattr(stub, name).argtypes is argtypes, name
