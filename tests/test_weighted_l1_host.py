"""NormL1 with a per-element lambda, host side: the Python oracle type against the CPU oracle's array arm, the lowering into
bz_problem_desc.g_lambda_vec, the field's place in the descriptor, and bz_problem_set_g_lambda's NULL-problem refusal from a C
program compiled against the header.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bazinga_hip.h")


def weights(n, seed=0):
    """0.5 U(0, 1) with exact zeros at the first index, the last one and one in the middle"""
    lam = 0.5 * np.random.default_rng(seed).uniform(0.0, 1.0, n)
    lam[[0, n // 2, n - 1]] = 0.0
    return lam


def test_constructor_takes_an_array_and_refuses_bad_ones(bz):
    lam = weights(7)
    g = bz.NormL1(lam)
    assert isinstance(g.lam, np.ndarray) and g.lam.shape == (7,) and np.array_equal(g.lam, lam)
    lam[1] = 9.0
    assert g.lam[1] != 9.0                                   # (its own copy)
    assert isinstance(bz.NormL1([0.0, 1.0]).lam, np.ndarray)
    assert type(bz.NormL1(2.5).lam) is float and type(bz.NormL1(np.float32(0.5)).lam) is float
    with pytest.raises(ValueError):
        bz.NormL1(np.array([0.1, -0.2, 0.3]))
    with pytest.raises(ValueError):
        bz.NormL1(np.array([0.1, np.nan, 0.3]))
    with pytest.raises(ValueError):
        bz.NormL1(np.array([0.1, np.inf]))
    with pytest.raises(ValueError):
        bz.NormL1(np.ones((2, 3)))
    with pytest.raises(ValueError):
        bz.NormL1(-1.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_prox_and_value_equal_the_oracle_exactly(bz, ref, dtype):
    n = 64
    lam = weights(n, 1)
    gamma = 0.37
    rng = np.random.default_rng(2)
    x = rng.standard_normal(n).astype(dtype)
    gl = dtype(gamma) * lam.astype(dtype)
    x[3], x[4], x[5], x[6], x[7] = np.nan, 0.0, -0.0, np.inf, -np.inf
    x[0], x[n - 1], x[n // 2] = np.nan, -0.0, np.inf         # ... and where lambda is zero
    x[10], x[11] = gl[10], -gl[11]                           # exactly at the threshold
    gd, gr = bz.NormL1(lam), ref.NormL1(lam)
    zd, zr = np.empty(n, dtype), np.empty(n, dtype)
    with np.errstate(invalid="ignore"):
        vd, vr = gd.prox(zd, x, gamma), gr.prox(zr, x, gamma)
    assert zd.dtype == dtype and np.array_equal(np.isnan(zd), np.isnan(zr)) and np.isnan(zr).sum() == 2
    assert np.array_equal(zd, zr, equal_nan=True)
    assert np.isnan(vd) and np.isnan(vr)
    # a finite input: the values themselves, and g(x)
    x = np.where(np.isfinite(x), x, dtype(0.25))
    vd, vr = gd.prox(zd, x, gamma), gr.prox(zr, x, gamma)
    assert np.array_equal(zd, zr) and vd == vr and np.isfinite(vr) and type(vd) is type(vr)
    assert zd[0] == x[0] and zd[n - 1] == x[n - 1] and zd[10] == 0 and zd[11] == 0
    assert gd(x) == gr(x)
    # the number arm is what it was
    zs = np.empty(n, dtype)
    gls = dtype(gamma * 0.3)
    vs = bz.NormL1(0.3).prox(zs, x, gamma)
    assert np.array_equal(zs, x + np.where(x <= -gls, gls, np.where(x >= gls, -gls, -x))) and vs == dtype(0.3) * np.sum(np.abs(zs))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_sets_the_vector_in_the_problems_type(bz, dtype):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    n = 9
    lam = weights(n, 3)
    rest = (bz.IdentityFunction(), bz.FreeSet())
    desc, keep = lower(bz.Zero(), bz.NormL1(lam), *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == L.BZ_G_NORM_L1 and desc.g_lambda_vec
    held = [a for a in keep if isinstance(a, np.ndarray) and a.ctypes.data == desc.g_lambda_vec]
    assert len(held) == 1 and held[0].dtype == dtype and np.array_equal(held[0], lam.astype(dtype))      # (kept alive)
    got = np.ctypeslib.as_array(C.cast(desc.g_lambda_vec, C.POINTER(C.c_double if dtype == np.float64 else C.c_float)), (n,))
    assert np.array_equal(got, lam.astype(dtype))
    with pytest.raises(ValueError):
        lower(bz.Zero(), bz.NormL1(lam[:-1]), *rest, n, n, np.dtype(dtype))
    desc, keep = lower(bz.Zero(), bz.NormL1(0.25), *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == L.BZ_G_NORM_L1 and not desc.g_lambda_vec and desc.g_lambda == 0.25
    # the slack form: n entries, the x half
    desc, keep = lower(bz.Zero(), bz.NormL1(lam[:8]), *rest, 8, 8, np.dtype(dtype), True)
    assert desc.g_lambda_vec and desc.slack == 1


def test_field_sits_between_g_hi_vec_and_c_A(bz):
    names = [f for f, _ in bz._lib.ProblemDesc._fields_]
    i = names.index("g_lambda_vec")
    assert names[i - 1] == "g_hi_vec" and names[i + 1] == "c_A"
    assert bz._lib.SIGNATURES["bz_problem_set_g_lambda"] == (C.c_int, [C.c_void_p, C.c_double, C.c_void_p])
    assert hasattr(bz.Problem, "set_g_lambda")


def test_setter_refuses_a_null_problem_from_c(bz):
    """a C99 program against the header and the library: BZ_ERR_ARG and a message, before any device call"""
    lib_dir = os.path.dirname(bz._lib.LIB_PATH)
    prog = f'''#include <stdio.h>
#include <string.h>
#include "{HEADER}"
int main(void) {{
    double lam[2] = {{0.0, 1.0}};
    int a = bz_problem_set_g_lambda(NULL, 0.5, NULL);
    int b = bz_problem_set_g_lambda(NULL, 0.0, lam);
    printf("%d %d %d %s\\n", a, b, BZ_ERR_ARG, bz_last_error());
    return 0;
}}
'''
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", src, "-o", exe, f"-L{lib_dir}", "-lbazinga_hip",
                               f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
        out = subprocess.check_output([exe], text=True).split(None, 3)
    assert out[0] == out[1] == out[2] == "-1" and "problem" in out[3]
