"""The two entry points of ZZZ_MG_PRODUCTS_ROWS (zzz_mg_products, zzz_mg_products_info) are new entry points and nothing else:
the header declares them, the library exports them, the Python mirror lists them, and neither the ABI version nor the options
struct moved."""
import ctypes
import os
import re

import zzz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zzz_mg_products", "zzz_mg_products_info")


def test_the_header_declares_the_library_exports_and_the_mirror_lists_the_entry_points():
    header = open(os.path.join(ROOT, "include", "zzz_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+zzz_mg_products\s*\(\s*zzz_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*\)\s*;", code)
    assert re.search(r"\bint\s+zzz_mg_products_info\s*\(\s*zzz_ctx\s*\*\s*ctx\s*,\s*int64_t\s+info\[8\]\s*\)\s*;", code)
    assert re.search(r"ZZZ_MG_PRODUCTS_LISTS\s*=\s*0\b", code) and re.search(r"ZZZ_MG_PRODUCTS_ROWS\s*=\s*1\b", code)
    assert (zzz.MG_PRODUCTS_LISTS, zzz.MG_PRODUCTS_ROWS) == (0, 1)
    lib = ctypes.CDLL(zzz.hip_lib_path())
    for n in NEW:
        assert hasattr(lib, n), f"libzzz_hip.so does not export {n}"
        assert zzz.ABI_SYMBOLS.count(n) == 1
    assert callable(zzz.Context.mg_products) and callable(zzz.Context.mg_products_info)


def test_the_abi_version_and_the_options_struct_did_not_move():
    header = open(os.path.join(ROOT, "include", "zzz_abi.h")).read()
    assert "#define ZZZ_ABI_VERSION 7" in header
    assert "zzz_mg_products and zzz_mg_products_info: new\n * entry points, version unchanged" in header
    assert ctypes.CDLL(zzz.hip_lib_path()).zzz_abi_version() == 7
    c = ctypes
    assert zzz.SolverOpts._fields_ == [
        ("variant", c.c_int32), ("pc", c.c_int32), ("norm", c.c_int32), ("op", c.c_int32), ("max_it", c.c_int32),
        ("profile", c.c_int32), ("single_reduction", c.c_int32), ("error_if_not_converged", c.c_int32), ("rtol", c.c_double),
        ("atol", c.c_double), ("dtol", c.c_double), ("pc_degree", c.c_int32), ("pc_esteig_its", c.c_int32), ("pc_ratio", c.c_double),
        ("pc_mg_levels", c.c_int32), ("pc_mg_coarse_eq_limit", c.c_int32)]
    assert c.sizeof(zzz.SolverOpts) == 80
    # the struct in the header: the same fields in the same order
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*zzz_solver_opts;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S)
    assert body and re.findall(r"\b(\w+)\s*;", body.group(1)) == [f[0] for f in zzz.SolverOpts._fields_]
