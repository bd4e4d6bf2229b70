#!/usr/bin/env python
"""Measure the sparse least-squares f (BZ_F_SPARSE_LEAST_SQUARES) on the MI355X.  bench.py is not involved.

    python tools/bench_sparse_ls.py --case lasso          # synth.sparse_lasso(m = 5e6, n = 1e7, k = 5), g = NormL1, c = Identity,
                                                          # D = Free, fp64: the two-launch form against BZ_SPLS_FUSED=0, and the
                                                          # two row kernels against the HBM peak
    python tools/bench_sparse_ls.py --case callback       # sparse_lasso(5e5, 1e6, 5): lowered kind against the callback kinds

Each case prints ONE JSON line and writes it to <out>/sparse_ls_<case>.json.  Per run: warm-up steps, then `repeats` timed
calls of bz_panoc_steps(K) (the call returns when its results are on the host): median, minimum and maximum it/s.  The
row kernels are timed by HIP events on their own dispatches (category 9); the two share that category, so the per-kernel
times come from a second run of the same worker under `rocprofv3 --kernel-trace --stats` (skipped with a note where that
tool is missing).  Every GPU step is a child process under a time limit of its own; the first one that fails ends the run."""
import argparse
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_sparse import HBM_PEAK, child, plan, run_problem      # noqa: E402
from tools.bench_sparse_qp import HostOnly, kernel_stats               # noqa: E402

KERNELS = ("k_spmv_ls_r", "k_spmv_ls_t_algrad", "k_spmv_ls_t")


def ls_bytes(f, dtype):
    """bytes of the passes over A_f and A_f' (DESIGN 4's model): both CSR arrays, the (virtual) row pointers, the
    virtual-row tables of a cut matrix, one gathered read, and per row b and r (k_spmv_ls_r) / x, mu, mu*y and the gradient
    (k_spmv_ls_t_algrad) / the product alone (k_spmv_ls_t)"""
    sz = np.dtype(dtype).itemsize
    tptr = np.concatenate(([0], np.cumsum(np.bincount(f.indices, minlength=f.n)))).astype(np.int64)
    out = {}
    for name, ptr, gathered, per_row, rows in (("k_spmv_ls_r", f.indptr, f.n, 2, f.m), ("k_spmv_ls_t_algrad", tptr, f.m, 4, f.n),
                                               ("k_spmv_ls_t", tptr, f.m, 1, f.n)):
        L, nv, seg = plan(ptr, f.nnz)
        out[name] = {"L": L, "segmented": seg,
                     "bytes": f.nnz * (sz + 4) + (nv + 1) * 8 + (nv * 8 if seg else 0) + gathered * sz + per_row * rows * sz}
    return out


def lasso(bz, m, n, k, dtype):
    d = bz.synth.sparse_lasso(m, n, k, dtype)
    f = bz.SparseLeastSquares(d["indptr"], d["indices"], d["data"], d["b"], n)
    return f, (bz.NormL1(0.1), bz.IdentityFunction(), bz.FreeSet())


def worker(args):
    import bazinga_jl_amd as bz
    dt = np.float64
    res = {"case": args.worker, "BZ_SPLS_FUSED": os.environ.get("BZ_SPLS_FUSED"), "dtype": "float64"}
    f, rest = lasso(bz, args.m, args.n, args.k, dt)
    res.update(m=f.m, n=f.n, nnz=f.nnz)
    if args.worker == "lasso":
        res["model"] = ls_bytes(f, dt)
        res["run"] = run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)
    else:
        res["lowered"] = run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)
        res["callback"] = run_problem(bz, (HostOnly(f),) + rest, f.n, f.n, dt, args.cb_steps, 3, 3, events=False)
        res["speedup"] = res["lowered"]["it_per_s_median"] / res["callback"]["it_per_s_median"]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["lasso", "callback"])
    ap.add_argument("--worker", choices=["lasso", "callback"])
    ap.add_argument("--m", type=int, default=None)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cb-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    args = ap.parse_args()
    small = (args.worker or args.case) == "callback"
    if args.n is None:
        args.n = 1_000_000 if small else 10_000_000
    if args.m is None:
        args.m = args.n // 2
    if args.worker:
        worker(args)
        return
    os.makedirs(args.out, exist_ok=True)
    base = [sys.executable, os.path.abspath(__file__), "--worker", args.case, "--m", str(args.m), "--n", str(args.n), "--k", str(args.k),
            "--steps", str(args.steps), "--cb-steps", str(args.cb_steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
    env = dict(os.environ)
    env.pop("BZ_SPLS_FUSED", None)
    env.pop("BZ_SPMV_L", None)
    if args.case == "lasso":
        res = {"case": "lasso", "two_launch": child(base, dict(env, BZ_SPLS_FUSED="1"), args.limit),
               "three_launch": child(base, dict(env, BZ_SPLS_FUSED="0"), args.limit)}
        a, b = res["two_launch"]["run"], res["three_launch"]["run"]
        res["two_over_three_launch"] = a["it_per_s_median"] / b["it_per_s_median"]
        res["spread_it_per_s"] = max(a["it_per_s_max"] - a["it_per_s_min"], b["it_per_s_max"] - b["it_per_s_min"])
        rocprof = shutil.which("rocprofv3")
        if rocprof:
            d = os.path.join(args.out, "rocprof_sparse_ls")
            shutil.rmtree(d, ignore_errors=True)
            short = list(base)
            short[short.index("--steps") + 1] = "40"
            short[short.index("--repeats") + 1] = "1"
            child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + short, dict(env, BZ_SPLS_FUSED="1"),
                  args.limit)
            ks = kernel_stats(d, KERNELS + ("k_spmv_fold",))
            shutil.rmtree(d, ignore_errors=True)
            for k, m in res["two_launch"]["model"].items():
                if k in ks:
                    ks[k]["bytes"] = m["bytes"]
                    ks[k]["fraction_of_8TBs"] = m["bytes"] / (ks[k]["avg_us"] * 1e-6) / HBM_PEAK
            res["per_kernel"] = ks
        else:
            res["per_kernel"] = "rocprofv3 not found: category 9 (both kernels together) only"
    else:
        res = child(base, env, args.limit)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, f"sparse_ls_{args.case}.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
