"""The C-ABI library loads and exports every symbol include/kimi_hip.h declares, and kimimaro_amd._abi binds it as the header
states it (no compute, no GPU).  _abi derives its tables from the header, so what is pinned here is spelled out literally."""
import ctypes as C
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kimi_hip.h")

i64, f32, f64, vp, ci, u32, u64 = C.c_int64, C.c_float, C.c_double, C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
# (restype, argtypes) as include/kimi_hip.h states them: together every entry of _abi's type map and both return types
SIGNATURES = {
    "kh_version": (ci, []),
    "kh_last_error": (ci, [C.c_char_p, ci]),
    "kh_edt": (ci, [vp, ci, i64, i64, i64, f32, f32, f32, ci, vp, vp, vp]),
    "kh_cross_sections": (ci, [vp, ci, i64, i64, i64, f64, f64, f64, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "kh_path_search": (ci, [vp, ci, vp, vp, i64, i64, i64, f32, f32, f32, vp, vp, vp, vp, u64, u64, vp, i64, vp, ci, vp]),
    "kh_region_apply_box": (ci, [vp, u32, i64, vp, vp, ci, i64, vp, vp]),
    "kh_host_join_plan": (i64, [i64, vp, vp, vp, vp, f64, ci, vp]),
    "kh_trace_paths": (ci, [vp, ci, vp, vp, vp, i64, i64, i64, f32, f32, f32, vp, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp,
                            vp, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
}
LABEL_FIELDS = [
    "segid", "list_offset", "count", "xmin", "xmax", "source", "max_loc", "max_val", "M", "root", "q_offset", "q_capacity",
    "heap_offset", "heap_capacity", "path_offset", "path_capacity", "tgt_offset", "n_before", "n_after", "max_paths", "n_paths",
    "n_vertices", "status", "stat_settled", "stat_heap_pushes", "cyc_target", "cyc_rail", "cyc_inval", "cyc_pop", "cyc_push",
    "cyc_fire", "soma_mode", "fsr", "soma_radius", "soma_scale", "soma_const", "nlev", "sweep_rmax", "ev_offset", "ev_chunks",
    "ev_shift", "stat_sweep_calls", "stat_sweep_bails", "stat_sweep_levels", "stat_sweep_events", "stat_sweep_why", "lev_window",
    "ev_spill", "stat_ghost_calls", "stat_rollbacks", "pdrf_log2e", "pdrf_scale", "stat_search_retries", "stat_search_spills",
    "stat_search_splits"]
LABEL_FLOATS = {"max_val", "M", "fsr", "soma_radius", "soma_scale", "soma_const", "sweep_rmax", "pdrf_scale"}
TRACE_FLAGS = {"TRACE_PROFILE": 1, "TRACE_HEAP_PRIO": 2, "TRACE_THREADS_64": 4, "TRACE_THREADS_128": 8, "TRACE_NO_GHOSTS": 16,
               "TRACE_GHOST_PARANOID": 32, "TRACE_BIG_LDS_HEAP": 64, "TRACE_VOXEL_GRAPH": 128, "TRACE_SCRATCH_POOL": 256,
               "TRACE_FUSED_EDF": 512}


def stripped_header():
    """the header without comments and preprocessor lines (this file's own reading, not _abi's)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)
    return re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)


def loaded_library():
    from kimimaro_amd import _abi, build
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_library_exports_header_symbols():
    from kimimaro_amd import _abi
    L = loaded_library()
    header = open(HEADER).read()
    declared = set(re.findall(r"\b(kh_[a-z0-9_]+)\s*\(", header))
    declared.discard("kh_label_t")
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(L, name), "libkimi_hip.so does not export %s" % name
    assert declared == set(_abi.SYMBOLS)
    assert L.kh_version() >= 100


def test_reader_consumes_every_prototype():
    """every `kh_name(...)` that a `;` follows at statement level is in SYMBOLS, once and in header order: a prototype that
    _abi's regular expression cannot read (nested parentheses, a return type on the line before) fails here instead of being left out"""
    from kimimaro_amd import _abi
    text, names = stripped_header(), []
    for m in re.finditer(r"\b(kh_\w+)\s*\(", text):
        depth, k = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[k], 0)
            k += 1
        if text[k:].lstrip().startswith(";"):
            names.append(m.group(1))
    assert len(names) == len(_abi.SYMBOLS) == len(set(names)) >= 76
    assert names == _abi.SYMBOLS == [name for name, _, _ in _abi.PROTOTYPES]


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature_matches_header(name):
    from kimimaro_amd import _abi
    restype, argtypes = SIGNATURES[name]
    assert [(r, a) for n, r, a in _abi.PROTOTYPES if n == name] == [(restype, argtypes)]


def test_every_function_is_bound():
    """after lib() every function carries the reader's argtypes and the return type its prototype states"""
    from kimimaro_amd import _abi
    L = loaded_library()
    stated = dict((name, ret) for ret, name in re.findall(r"\b(int64_t|int)\s+(kh_\w+)\s*\(", stripped_header()))
    assert set(stated) == set(_abi.SYMBOLS)
    for name, _, argtypes in _abi.PROTOTYPES:
        f = getattr(L, name)
        assert f.argtypes is not None and list(f.argtypes) == argtypes, name
        assert f.restype is {"int": ci, "int64_t": i64}[stated[name]], name
    for name, (restype, argtypes) in SIGNATURES.items():
        assert (getattr(L, name).restype, list(getattr(L, name).argtypes)) == (restype, argtypes), name
    assert sorted(n for n in stated if stated[n] == "int64_t") == [
        "kh_cross_sections_scratch_bytes", "kh_host_ccl26", "kh_host_consolidate_paths", "kh_host_enclosed_regions",
        "kh_host_find_border_targets", "kh_host_join_plan", "kh_host_merge_components", "kh_host_resolve_holes"]


def test_readers_are_closed():
    """what the readers do not know raises, naming the function (or define, or member) and the type: nothing defaults to int"""
    from kimimaro_amd import _abi
    good = "#define KH_A 16\n#define KH_B 1u /* c */\n#define KH_C 0x100 // c\n#define KH_D (-2)\n" \
           "typedef struct kh_t { uint32_t a, b; /* c */ float c; } kh_t;\n" \
           "int kh_f(const char* s, char* buf, const uint64_t* p, uint64_t v, double d);\nint64_t kh_g(void);\n"
    assert _abi.header_prototypes(good) == [("kh_f", ci, [C.c_char_p, C.c_char_p, vp, u64, f64]), ("kh_g", i64, [])]
    assert _abi.header_defines(good) == {"KH_A": 16, "KH_B": 1, "KH_C": 256, "KH_D": -2}
    assert _abi.header_struct(good, "kh_t") == [("a", "<u4"), ("b", "<u4"), ("c", "<f4")]
    with pytest.raises(TypeError, match=r"kh_f has a parameter 'size_t n'"):
        _abi.header_prototypes("int kh_ok(int a);\nint kh_f(void* p, size_t n);\nint kh_g(void);\n")
    with pytest.raises(TypeError, match=r"kh_f returns 'float'"):
        _abi.header_prototypes("int kh_ok(int a);\nfloat kh_f(int a);\nint kh_g(void);\n")
    with pytest.raises(TypeError, match=r"kh_f returns 'unsigned int'"):
        _abi.header_prototypes("unsigned int kh_f(int a);\n")
    with pytest.raises(TypeError, match=r"kh_f has a parameter 'int a\[3\]'"):
        _abi.header_prototypes("int kh_f(int a[3]);\n")
    with pytest.raises(TypeError, match=r"kh_t has a member 'uint16_t b'"):
        _abi.header_struct("typedef struct kh_t {\n  uint32_t a; uint16_t b;\n} kh_t;\n", "kh_t")
    with pytest.raises(TypeError, match=r"kh_t has a member 'uint32_t a\[4\]'"):
        _abi.header_struct("typedef struct kh_t { uint32_t a[4]; } kh_t;", "kh_t")
    for value in ("(1 << 4)", "KH_A", "1.5f", "-1", ""):
        with pytest.raises(ValueError, match=r"#define KH_X has a value"):
            _abi.header_defines("#define KH_A 1\n#define KH_X %s\nint kh_g(void);\n" % value)


def test_missing_header_is_reported_with_its_path(tmp_path):
    from kimimaro_amd import _abi
    os.mkdir(str(tmp_path / "pkg"))
    copy = shutil.copy(_abi.__file__, str(tmp_path / "pkg" / "_abi.py"))
    spec = importlib.util.spec_from_file_location("abi_without_header", copy)
    with pytest.raises(RuntimeError) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "HipUnavailableError" and str(tmp_path / "include" / "kimi_hip.h") in str(e.value)
    assert _abi.HEADER_PATH == HEADER


def test_label_struct_matches_header():
    from kimimaro_amd import _abi
    header = open(HEADER).read()
    body = header[header.index("typedef struct kh_label_t {"):header.index("} kh_label_t;")]
    fields = re.findall(r"\b(?:uint32_t|float)\s+([A-Za-z_0-9, ]+);", body)
    names = [n.strip() for f in fields for n in f.split(",")]
    assert names == LABEL_FIELDS == list(_abi.LABEL_T.names)
    assert [n for n in names if _abi.LABEL_T[n] == "<f4"] == [n for n in names if n in LABEL_FLOATS]
    assert all(_abi.LABEL_T[n] == ("<f4" if n in LABEL_FLOATS else "<u4") for n in names)
    # every member is one 32-bit word, and the searches' regime counters were appended: no earlier offset moved
    assert _abi.LABEL_T.itemsize == 4 * len(names) == 220
    assert [_abi.LABEL_T.fields[n][1] for n in names] == list(range(0, 220, 4))
    assert names[-3:] == ["stat_search_retries", "stat_search_spills", "stat_search_splits"]
    assert _abi.LABEL_T.fields["pdrf_scale"][1] == 204


def test_trace_flags_match_header():
    """every KH_TRACE_* flag of the header has its twin in _abi, with the header's value -- the value outside binders see"""
    from kimimaro_amd import _abi
    header = open(HEADER).read()
    names = set(re.findall(r"^#define KH_(TRACE_\w+)", header, re.M))
    defines = {name: int(value, 0) for name, value in re.findall(r"^#define KH_(TRACE_\w+)[ \t]+(\d+|0[xX][0-9a-fA-F]+)\b", header, re.M)}
    assert len(names) >= 10 and names == set(defines), "KH_TRACE_* defines this test cannot read: %s" % sorted(names - set(defines))
    for name, value in defines.items():
        assert hasattr(_abi, name), "kimimaro_amd._abi lacks %s" % name
        assert getattr(_abi, name) == value, name
    assert defines == TRACE_FLAGS
    assert {name: getattr(_abi, name) for name in TRACE_FLAGS} == TRACE_FLAGS


def test_constants_have_their_abi_values():
    """the other values of include/kimi_hip.h that INTEGRATION.md's binders compile in: a change must fail here, not flow through"""
    from kimimaro_amd import _abi
    assert (_abi.PDRF_BASE, _abi.PDRF_FINISH, _abi.PDRF_KEEP_OTHERS) == (-1, -2, 0x100)
    assert (_abi.HOLES_PROCESSED, _abi.HOLES_FILLED, _abi.HOLES_KILLED) == (1, 2, 4)
    assert _abi.BRICK == (64, 4, 4)
    assert _abi.SWEEP_LDS_LEVELS == 16384
    assert _abi.GRAPH_LDS_PAIRS == 2048
    assert _abi.ENODEVICE == 3
    assert list(_abi.ST_BITS) == [1, 2, 4, 8, 16, 32] and all(type(k) is int for k in _abi.ST_BITS)
    assert _abi.describe_status(0) == "ok" and _abi.describe_status(2 | 16) == \
        "invalidation heap overflow, float-absorption plateau while back-tracking"
    assert (_abi.SWEEP_MAX_LEVELS, _abi.NO_FEATURE) == (1 << 22, 0xFFFFFFFF)       # no #define in the header: literals in _abi


def test_product_fails_loudly_without_gpu():
    import numpy as np
    import torch
    import kimimaro_amd
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.skeletonize(np.ones((16, 16, 16), np.uint32), dust_threshold=0)


def test_product_never_imports_oracle():
    """The product path must not route through the oracle (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "kimimaro_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M), fn
