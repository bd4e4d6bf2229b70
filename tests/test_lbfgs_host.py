"""The L-BFGS memory's host arithmetic (bazinga.jl_amd/csrc/bz_lbfgs_host.h) against the oracle, without a GPU.

The header is host-only: a stand-alone program drives LbfgsMemory<double> and LbfgsMemory<float> through inserts, a ring
overflow and a reset with numbers computed here, and prints the ring and the compact form's coefficients as hex floats.
They are the same loops in the same order in double as `LBFGSCompactOperator` of oracle/bazinga_ref.py, so the
comparison is `==`: a difference means the arithmetic is no longer the oracle's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bazinga.jl_amd", "csrc", "bz_lbfgs_host.h")
CM = 5
N = 8

DRIVER = r'''
#include "bz_lbfgs_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

using namespace bz;

static double num(std::istream& in) { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); }
static void row(const char* name, const double* v, int n) {
    std::printf(" %s", name);
    for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
}
template <class T> static void show(const LbfgsMemory<T>& mem, bool anderson) {
    double H0, u1[CM], u2h[CM], M1[CM * CM], M2[CM * CM];
    mem.coefficients(anderson, H0, u1, u2h);
    mem.compact_matrices((double)mem.H, M1, M2);
    std::printf("H %a gm %d spare %d order %d", (double)mem.H, mem.gm, mem.spare, (int)mem.order.size());
    for (int s : mem.order) std::printf(" %d", s);
    row("M1", M1, CM * CM); row("M2", M2, CM * CM); row("u1", u1, CM); row("u2h", u2h, CM);
    std::printf(" H0 %a\n", H0);
}
// commands:  new M | reset | ins anderson ys yty m sy[m] yy[m] p[m] w[m] p_new w_new | pw m p[m] w[m] anderson
template <class T> static int run(std::istream& in) {
    LbfgsMemory<T> mem;
    std::string cmd;
    while (in >> cmd) {
        if (cmd == "new") { int M; in >> M; mem.reset_all(M); }
        else if (cmd == "reset") mem.reset();
        else if (cmd == "ins") {
            int anderson, m;
            in >> anderson;
            const T ys = (T)num(in), yty = (T)num(in);
            in >> m;
            double sy[CM] = {0}, yy[CM] = {0};
            for (int i = 0; i < m; ++i) sy[i] = num(in);
            for (int i = 0; i < m; ++i) yy[i] = num(in);
            // (as the solver's commit: p, w of the stored pairs at the new state, zero beyond them, and the new pair's)
            for (int i = 0; i < CM; ++i) mem.hp[i] = i < m ? num(in) : 0.0;
            for (int i = 0; i < CM; ++i) mem.hw[i] = i < m ? num(in) : 0.0;
            mem.p_new = num(in); mem.w_new = num(in); mem.pw_valid = true;
            mem.insert(ys, yty, sy, yy, true, anderson != 0);
            show(mem, anderson != 0);
        } else if (cmd == "pw") {
            int m, anderson;
            in >> m;
            for (int i = 0; i < CM; ++i) mem.hp[i] = i < m ? num(in) : 0.0;
            for (int i = 0; i < CM; ++i) mem.hw[i] = i < m ? num(in) : 0.0;
            in >> anderson;
            show(mem, anderson != 0);
        } else return 2;
    }
    return 0;
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[2]);
    return std::strcmp(argv[1], "f32") == 0 ? run<float>(in) : run<double>(in);
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("lbfgs_host")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)

    def run(dtype, script):
        f = d / "script.txt"
        f.write_text(script)
        out = subprocess.run([str(exe), "f32" if dtype == np.float32 else "f64", str(f)], check=True, capture_output=True,
                             text=True).stdout
        return [_parse(line) for line in out.splitlines()]
    return run


def _parse(line):
    t = line.split()
    rec, i = {}, 0
    while i < len(t):
        key = t[i]
        if key in ("gm", "spare"):
            rec[key] = int(t[i + 1]); i += 2
        elif key in ("H", "H0"):
            rec[key] = float.fromhex(t[i + 1]); i += 2
        elif key == "order":
            k = int(t[i + 1])
            rec[key] = [int(v) for v in t[i + 2:i + 2 + k]]; i += 2 + k
        else:
            k = CM * CM if key in ("M1", "M2") else CM
            rec[key] = np.array([float.fromhex(v) for v in t[i + 1:i + 1 + k]]); i += 1 + k
    return rec


def _hx(vals):
    return " ".join(float(v).hex() for v in vals)


def _spd(rng):
    A = rng.standard_normal((N, N))
    return A @ A.T + N * np.eye(N)


def test_header_is_host_only():
    text = open(HEADER).read()
    assert "#include <hip" not in text and "rccl" not in text


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [1, 3, 5])
def test_ring_and_compact_coefficients_equal_the_oracle(driver, ref, dtype, M):
    """2M + 2 inserts of pairs (s, y = B s), B SPD, with one reset after insert M + 1: after every insert H, the Gram
    size, the ring order, M1, M2, u1 and u2h = H0 u2 equal the oracle's, bit for bit."""
    rng = np.random.default_rng(1234 + M)
    B = _spd(rng).astype(dtype)
    op = ref.LBFGSCompactOperator(M, np.zeros(N, dtype=dtype))
    script, expect = [f"new {M}"], []
    for k in range(2 * M + 2):
        s = rng.standard_normal(N).astype(dtype)
        y = (B @ s).astype(dtype)
        m = op.currmem
        # the numbers the device would have measured: Gram rows of the new pair against the stored ones (the oracle's own
        # dot products), p = S'v and w = Y'v of the stored pairs and of the new one (any numbers: random)
        ys, yty = ref._dot(s, y), ref._dot(y, y)
        sy = [float(ref._dot(op.S[i], y)) for i in range(m)]
        yy = [float(ref._dot(op.Y[i], y)) for i in range(m)]
        p, w = rng.standard_normal(m + 1), rng.standard_normal(m + 1)
        script.append(f"ins 0 {_hx([ys, yty])} {m} {_hx(sy)} {_hx(yy)} {_hx(p[:m])} {_hx(w[:m])} {_hx([p[m], w[m]])}")
        assert op.update(s, y) > 0
        if m == M:                                       # the oldest pair was overwritten: its p, w leave with it
            p, w = p[1:], w[1:]
        H0 = float(op.H)
        M1, M2 = op.coefficient_matrices(op.SY, op.YY, H0)
        u1, u2 = op.coefficients(M1, M2, H0, list(p), list(w))
        expect.append((float(op.H), op.currmem, M1, M2, u1, [H0 * v for v in u2]))
        if k == M:                                       # (after insert M + 1: the ring has overflowed once)
            op.reset()
            script.append("reset")
    got = driver(dtype, "\n".join(script) + "\n")
    assert len(got) == len(expect) == 2 * M + 2
    for g, (H, m, M1, M2, u1, u2h) in zip(got, expect):
        assert g["H"] == H and g["H0"] == H and g["gm"] == m
        assert len(g["order"]) == m and len(set(g["order"]) | {g["spare"]}) == m + 1
        assert all(0 <= slot <= M for slot in g["order"] + [g["spare"]])
        pad1, pad2 = np.zeros((CM, CM)), np.zeros((CM, CM))
        pad1[:m, :m], pad2[:m, :m] = M1, M2
        assert np.array_equal(g["M1"].reshape(CM, CM), pad1)
        assert np.array_equal(g["M2"].reshape(CM, CM), pad2)
        assert np.array_equal(g["u1"], np.array(list(u1) + [0.0] * (CM - m)))
        assert np.array_equal(g["u2h"], np.array(list(u2h) + [0.0] * (CM - m)))
    # the ring itself: a new pair goes to the slot that was spare, the others keep their places, newest first; a reset
    # empties it
    prev, prev_spare = [], 0
    for k, g in enumerate(got):
        assert g["order"][0] == prev_spare and g["order"][1:] == prev[:M - 1]
        prev, prev_spare = ([], g["spare"]) if k == M else (g["order"], g["spare"])


def _anderson(driver, Y, w):
    """the coefficients for the pairs' y vectors Y (rows) and the right-hand side w, and the Gram matrix they solve"""
    m = Y.shape[0]
    script = ["new 5"]
    for j in range(m):
        yy = [float(np.dot(Y[i], Y[j])) for i in range(j)]
        zeros = [0.0] * j
        script.append(f"ins 1 {_hx([1.0, float(np.dot(Y[j], Y[j]))])} {j} {_hx(zeros)} {_hx(yy)} {_hx(zeros)} {_hx(zeros)} {_hx([0.0, 0.0])}")
    script.append(f"pw {m} {_hx([0.0] * m)} {_hx(w)} 1")
    g = driver(np.float64, "\n".join(script) + "\n")[-1]
    assert g["H0"] == 1.0 and np.array_equal(g["u2h"], -g["u1"]) and np.all(g["u1"][m:] == 0.0)
    G = np.array([[float(np.dot(Y[min(i, j)], Y[max(i, j)])) for j in range(m)] for i in range(m)])
    return g["u1"][:m], G


@pytest.mark.parametrize("m", [1, 3, 5])
def test_anderson_coefficients_solve_a_full_rank_gram_system(driver, m):
    rng = np.random.default_rng(77 + m)
    Y = rng.standard_normal((m, N))
    w = Y @ rng.standard_normal(N)
    a, G = _anderson(driver, Y, w)
    assert np.max(np.abs(G @ a - w)) <= 1e-12 * np.max(np.abs(w))


@pytest.mark.parametrize("m,dup", [(3, (0, 2)), (5, (1, 4)), (5, (3, 4))])
def test_anderson_coefficients_with_a_duplicated_pair(driver, m, dup):
    """rank m - 1: exactly one coefficient is zero, the others solve the system without that pair"""
    rng = np.random.default_rng(99 + m)
    Y = rng.standard_normal((m, N))
    Y[dup[1]] = Y[dup[0]]
    w = Y @ rng.standard_normal(N)
    a, G = _anderson(driver, Y, w)
    zero = np.flatnonzero(a == 0.0)
    assert len(zero) == 1 and zero[0] in dup
    keep = [i for i in range(m) if i != zero[0]]
    assert np.max(np.abs(G[np.ix_(keep, keep)] @ a[keep] - w[keep])) <= 1e-12 * np.max(np.abs(w))
