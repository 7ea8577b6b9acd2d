"""The C-ABI library loads without a GPU and exports every symbol include/pdmssd_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdmssd_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pdm_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_reference_extension_surface():
    names = declared_symbols()
    # the nine functions of pointnet2_api.cpp:10-24, under their pdm_ names
    for n in ["pdm_ball_query", "pdm_group_points", "pdm_group_points_grad", "pdm_gather_points",
              "pdm_gather_points_grad", "pdm_furthest_point_sampling", "pdm_three_nn", "pdm_three_interpolate",
              "pdm_three_interpolate_grad"]:
        assert n in names


def test_library_loads_and_exports_every_declared_symbol():
    from pdm_ssd_amd import _native
    lib = _native.lib()
    assert lib.pdm_abi_version() == _native.ABI_VERSION
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} declared in include/pdmssd_hip.h but not exported"
    # and the Python binding covers the header: it is derived from it, so "bound" means "declared"
    bound = set(_native.EXPORTS)
    assert set(declared_symbols()) <= bound, set(declared_symbols()) - bound
    assert bound == set(declared_symbols()), bound - set(declared_symbols())


def test_extension_module_mirrors_reference_function_table():
    from pdm_ssd_amd.pointnet2_batch import pointnet2_batch_hip as ext
    for n in ["ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper", "gather_points_wrapper",
              "gather_points_grad_wrapper", "farthest_point_sampling_wrapper", "three_nn_wrapper",
              "three_interpolate_wrapper", "three_interpolate_grad_wrapper"]:
        assert callable(getattr(ext, n))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from pdm_ssd_amd import _native
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_native.NativeLibraryError):
        _native.lib()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "pdm_ssd_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "libpdmssd_oracle" not in src, f


def test_new_entry_points_validate_their_arguments_before_any_launch():
    """Round-4 entry points return an error code + message for arguments they cannot serve (no GPU is touched: the checks
    come first), as the rest of the ABI does instead of the reference's exit(-1)."""
    import ctypes as C

    from pdm_ssd_amd import _native
    lib = _native.lib()
    dims_ok = (C.c_int * 4)(128, 256, 256, 16)
    dims_bad = (C.c_int * 4)(128, 128, 128, 16)
    assert lib.pdm_rows_mlp_x3_stream_bytes(3, C.cast(dims_ok, C.c_void_p)) == 25 * 24 * 1024
    assert lib.pdm_rows_mlp_x3_stream_bytes(3, C.cast(dims_bad, C.c_void_p)) == 0
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    with pytest.raises(_native.NativeLibraryError, match="only 128 -> 256 -> 256"):
        _native.call("pdm_rows_mlp_x3", 0, 64, 128, ptr, 3, C.cast(dims_bad, C.c_void_p), ptr, 1 << 20, ptr, 0, ptr, 16, 8)
    with pytest.raises(_native.NativeLibraryError, match="weight stream"):
        _native.call("pdm_rows_mlp_x3", 0, 64, 128, ptr, 3, C.cast(dims_ok, C.c_void_p), ptr, 1024, ptr, 0, ptr, 16, 8)
    assert lib.pdm_point_head_loss_workspace_bytes(1000) == 16 + 4 * 2 * 4
    with pytest.raises(_native.NativeLibraryError, match="multiple of n_per_sample"):
        _native.call("pdm_point_head_loss", 0, 1000, 300, 4, 3, 3, 0, ptr, 3, ptr, 8, ptr, 4, ptr, ptr, ptr, ptr, ptr, 0.1, 0.25, 2.0, 1.0, 1.0,
                     ptr, ptr, ptr, ptr, ptr, 1 << 20)
    with pytest.raises(_native.NativeLibraryError, match="workspace too small"):
        _native.call("pdm_point_head_loss", 0, 1000, 500, 4, 3, 3, 0, ptr, 3, ptr, 8, ptr, 4, ptr, ptr, ptr, ptr, ptr, 0.1, 0.25, 2.0, 1.0, 1.0,
                     ptr, ptr, ptr, ptr, ptr, 8)



LITERAL_HEADER = """
#ifndef X_H
#define X_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PDM_E_BADARG (-1)   /* negative size (or a null pointer) */
/* returns the text of the last error ( thread-local ) */
const char *pdm_last_error(void);
int pdm_abi_version(void);
size_t pdm_ws_bytes(int n, long long rows);   // trailing comment with pdm_not_a_function(int)
/* a comment with a call-like text: pdm_fake(int a,
 * float b); and a parenthesis ( in it ) */
int pdm_many(void *stream, int count, const float *const *src, void *const *dst, const size_t *bytes,
             unsigned seed, unsigned int flags, long long n,
             size_t ws_bytes, double overlap, float eps,
             unsigned long long *slot, const unsigned long long total);
int pdm_tune_knob(int);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_maps_every_type_of_the_header():
    import ctypes as C

    from pdm_ssd_amd import _native
    got = _native.parse_header(LITERAL_HEADER)
    assert got == {
        "pdm_last_error": (C.c_char_p, []),
        "pdm_abi_version": (C.c_int, []),
        "pdm_ws_bytes": (C.c_size_t, [C.c_int, C.c_longlong]),
        "pdm_many": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_longlong,
                               C.c_size_t, C.c_double, C.c_float, C.c_void_p, C.c_ulonglong]),
        "pdm_tune_knob": (C.c_int, [C.c_int]),
    }


@pytest.mark.parametrize("proto, words", [
    ("int pdm_f(void *stream, short n);", ("pdm_f", "short n")),
    ("int pdm_g(int n, struct box b);", ("pdm_g", "struct box b")),
    ("float pdm_h(int n);", ("pdm_h", "float")),
])
def test_parser_refuses_a_type_it_does_not_know(proto, words):
    from pdm_ssd_amd import _native
    with pytest.raises(_native.NativeLibraryError) as e:
        _native.parse_header(proto)
    for w in words:
        assert w in str(e.value)


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    from pdm_ssd_amd import _native
    missing = str(tmp_path / "nope.h")
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "_declared", None)
    monkeypatch.setattr(_native, "HEADER_PATH", missing)
    with pytest.raises(_native.NativeLibraryError, match="nope.h"):
        _native.lib()


def test_every_declared_function_is_bound_as_the_header_says():
    from pdm_ssd_amd import _native
    lib = _native.lib()
    want = _native.parse_header(open(HEADER).read())
    assert sorted(want) == declared_symbols() and len(want) >= 187
    for name, (restype, argtypes) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes), name
        assert list(fn.argtypes) == argtypes, name
    assert os.path.samefile(_native.HEADER_PATH, HEADER)


def test_every_extern_c_definition_is_declared():
    """What catches the next entry point or tuning knob that is defined and called but missing from the header."""
    csrc = os.path.join(ROOT, "pdm_ssd_amd", "csrc")
    defined = set()
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            defined |= set(re.findall(r'extern\s+"C"[^;{()]*?\b(pdm_[a-z0-9_]+)\s*\(', open(os.path.join(csrc, f)).read()))
    from pdm_ssd_amd import _native
    raw = ctypes.CDLL(_native.LIB_PATH)
    defined = {n for n in defined if hasattr(raw, n)}      # (a definition inside an #if of a diagnostic build is not in the library)
    assert len(defined) >= 187
    assert defined <= set(declared_symbols()), sorted(defined - set(declared_symbols()))
