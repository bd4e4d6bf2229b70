"""The CSR transpose of the sparse kinds (bazinga.jl_amd/csrc/bz_csr_host.h) without a GPU.

The header is host-only: a stand-alone program reads a CSR matrix, calls csr_transpose<double> / <float> and prints the
transpose's arrays.  They must equal the stable counting sort stated here with numpy: a column's entries in ascending row
order, those of one row in stored order — the order in which the row kernels add A'v, so it fixes the bits of a gradient."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_sparse import csr_of, structured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bazinga.jl_amd", "csrc", "bz_csr_host.h")

DRIVER = r'''
#include "bz_csr_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

template <class T> static int run(std::istream& in) {
    long long rows, cols, nnz;
    in >> rows >> cols >> nnz;
    std::vector<int64_t> rp((size_t)rows + 1), tp;
    std::vector<int32_t> col((size_t)nnz), tcol;
    std::vector<T> val((size_t)nnz), tval;
    for (auto& v : rp) { long long t; in >> t; v = t; }
    for (auto& v : col) { long long t; in >> t; v = (int32_t)t; }
    for (auto& v : val) { std::string t; in >> t; v = (T)std::strtod(t.c_str(), nullptr); }
    bz::csr_transpose<T>(rows, cols, rp, col, val, tp, tcol, tval);
    if ((long long)tp.size() != cols + 1 || (long long)tcol.size() != nnz || (long long)tval.size() != nnz) return 3;
    for (auto v : tp) std::printf("%lld ", (long long)v);
    std::printf("\n");
    for (auto v : tcol) std::printf("%d ", (int)v);
    std::printf("\n");
    for (auto v : tval) std::printf("%a ", (double)v);
    std::printf("\n");
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
    d = tmp_path_factory.mktemp("csr_host")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)

    def run(dtype, rows, cols, indptr, indices, data):
        f = d / "matrix.txt"
        f.write_text(f"{rows} {cols} {len(indices)}\n" + " ".join(map(str, indptr)) + "\n" + " ".join(map(str, indices)) + "\n" +
                     " ".join(float(v).hex() for v in data) + "\n")
        out = subprocess.run([str(exe), "f32" if dtype == np.float32 else "f64", str(f)], check=True, capture_output=True,
                             text=True).stdout.split("\n")
        return (np.array(out[0].split(), np.int64), np.array(out[1].split(), np.int64),
                np.array([float.fromhex(v) for v in out[2].split()]))
    return run


def test_header_is_host_only():
    text = open(HEADER).read()
    assert "#include <hip" not in text and "bz_kernels" not in text


def stable_transpose(rows, cols, indptr, indices, data):
    r = np.repeat(np.arange(rows), np.diff(indptr))
    order = np.argsort(indices, kind="stable")                 # entries are stored by ascending row: stable keeps that order
    tp = np.concatenate(([0], np.cumsum(np.bincount(indices, minlength=cols)))).astype(np.int64)
    return tp, r[order], data[order]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(3, 70, 0.5), (41, 121, 0.1), (121, 41, 0.5), (257, 1031, 0.03)])
def test_transpose_is_the_stable_counting_sort(driver, shape, dtype):
    rows, cols, p = shape
    A = structured(rows, cols, p, np.random.default_rng(rows + cols), False, dtype)      # a full and an empty row and column
    indptr, indices, data = csr_of(A, np.random.default_rng(1))                          # unsorted rows
    k = int(indptr[2])                                                                   # a duplicated entry, adjacent
    indices, data = np.insert(indices, k, indices[k]), np.insert(data, k, dtype(7))
    indptr[3:] += 1
    tp, tcol, tval = driver(dtype, rows, cols, indptr, indices, data)
    ep, ecol, eval_ = stable_transpose(rows, cols, indptr, indices, data)
    assert np.array_equal(tp, ep) and np.array_equal(tcol, ecol) and np.array_equal(tval, eval_.astype(np.float64))
    at = int(tp[indices[k]]) + int(np.flatnonzero(tcol[tp[indices[k]]:tp[indices[k] + 1]] == 2)[0])
    assert tval[at] == 7 and tcol[at + 1] == 2 and tval[at + 1] == float(data[k + 1])   # the duplicates keep their stored order


def test_transpose_of_empty_matrices(driver):
    tp, tcol, tval = driver(np.float64, 4, 3, np.zeros(5, np.int64), np.zeros(0, np.int64), np.zeros(0))
    assert np.array_equal(tp, np.zeros(4)) and tcol.size == 0 and tval.size == 0
    tp, tcol, tval = driver(np.float64, 1, 1, np.array([0, 1]), np.array([0]), np.array([2.5]))
    assert np.array_equal(tp, [0, 1]) and np.array_equal(tcol, [0]) and np.array_equal(tval, [2.5])
