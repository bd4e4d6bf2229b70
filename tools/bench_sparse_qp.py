#!/usr/bin/env python
"""Measure the sparse quadratic f (BZ_F_SPARSE_QUADRATIC) on the MI355X.  bench.py is not involved.

    python tools/bench_sparse_qp.py --case laplacian      # the 2048^2 Laplacian as CSR, c = Identity, fp64: the one-launch
                                                          # form against BZ_SPQ_FUSED=0 and against Stencil5ptQuadratic
    python tools/bench_sparse_qp.py --case callback       # the 1000^2 Laplacian: lowered kind against the callback kinds
    python tools/bench_sparse_qp.py --case qp             # synth.sparse_qp(n ~ 1e7 / 3) beside a sparse c: three row kernels

Each case prints ONE JSON line and writes it to <out>/sparse_qp_<case>.json.  Per run: warm-up steps, then `repeats` timed
calls of bz_panoc_steps(K) (the call returns when its results are on the host): median, minimum and maximum it/s.  The
row kernels are timed by HIP events on their own dispatches (category 9); with c = Identity the pass over Q is that
category's only kernel.  Beside a sparse c three kernels share it, so the per-kernel times come from a second run of the
same worker under `rocprofv3 --kernel-trace --stats` (skipped with a note where that tool is missing).  Every GPU step is a
child process under a time limit of its own; the first one that fails ends the run."""
import argparse
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_sparse import HBM_PEAK, child, pass_bytes, plan, run_problem      # noqa: E402


class HostOnly:
    """hides the type of the lowered f: the problem then runs through the callback kinds, evaluating the same CSR arrays on
    the host with numpy"""

    def __init__(self, f):
        self.gradient = f.gradient


def q_bytes(f, dtype, per_row):
    """bytes of one pass over Q (DESIGN 4's model): both CSR arrays, the (virtual) row pointers, the virtual-row tables of a
    cut matrix, one gathered read of x, `per_row` vectors of n"""
    sz = np.dtype(dtype).itemsize
    L, nv, seg = plan(f.indptr, f.nnz)
    return {"L": L, "segmented": seg, "bytes": f.nnz * (sz + 4) + (nv + 1) * 8 + (nv * 8 if seg else 0) + f.n * sz + per_row * f.n * sz}


def laplacian(bz, nx, dtype):
    """cfg 3's data (synth.obstacle_grid) with the matrix as CSR: q = -b, g = NormL1(0.1 h^2), D = Box[psi, inf)"""
    d = bz.synth.obstacle_grid(nx, nx, dtype)
    lap = bz.synth.laplacian_2d(nx, nx, dtype)
    f = bz.SparseQuadratic(lap["indptr"], lap["indices"], lap["data"], -d["b"], check_symmetric=False)
    rest = (bz.NormL1(0.1 * float(d["b"][0])), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(d["psi"], np.inf)))
    return d, f, rest


def kernel_stats(directory, names):
    import csv
    import glob
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in names:
                if k + "<" in row.get("Name", "").replace("void bz::", "").replace(" ", "") and row.get("Calls"):
                    a = out.setdefault(k, {"calls": 0, "total_ns": 0.0})
                    a["calls"] += int(row["Calls"]); a["total_ns"] += float(row.get("TotalDurationNs") or 0.0)
    return {k: {"calls": v["calls"], "avg_us": v["total_ns"] / v["calls"] / 1e3} for k, v in out.items() if v["calls"]}


def worker(args):
    import bazinga_jl_amd as bz
    dt = np.float64
    res = {"case": args.worker, "BZ_SPQ_FUSED": os.environ.get("BZ_SPQ_FUSED"), "dtype": "float64"}
    run = lambda dev, n, ny, **kw: run_problem(bz, dev, n, ny, dt, kw.pop("K", args.steps), args.warmup, args.repeats, **kw)
    if args.worker == "laplacian":
        d, f, rest = laplacian(bz, args.nx, dt)
        n = f.n
        res.update(n=n, nnz=f.nnz)
        if args.form == "stencil":
            res["run"] = run((bz.Stencil5ptQuadratic(args.nx, args.nx, d["b"]),) + rest, n, n, events=False)
        else:
            res["model"] = q_bytes(f, dt, 6)      # x, q, mu, mu*y, the lower bound of D, the gradient
            res["run"] = run((f,) + rest, n, n)
    elif args.worker == "callback":
        d, f, rest = laplacian(bz, args.nx, dt)
        n = f.n
        res.update(n=n, nnz=f.nnz)
        res["lowered"] = run((f,) + rest, n, n)
        res["callback"] = run_problem(bz, (HostOnly(f),) + rest, n, n, dt, args.cb_steps, 3, 3, events=False)
        res["speedup"] = res["lowered"]["it_per_s_median"] / res["callback"]["it_per_s_median"]
    else:
        d = bz.synth.sparse_qp(args.n, args.n // 10, dtype=dt)
        f = bz.SparseQuadratic(d["Q_indptr"], d["Q_indices"], d["Q_data"], d["fq"], check_symmetric=False)
        c = bz.SparseAffine(d["indptr"], d["indices"], d["data"], d["b"], args.n)
        res.update(n=args.n, ny=c.ny, nnz_Q=f.nnz, nnz_A=c.nnz)
        res["model"] = [q_bytes(f, dt, 1)] + pass_bytes(c, dt, 6, 4)      # Q x | b, mu, mu*y, lo, hi, yhat | x, Q x, q, grad
        res["run"] = run((f, bz.IndBox(0.0, 1.0), c, bz.ClosedSet(bz.IndBox(d["lo"], d["hi"]))), args.n, c.ny)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["laplacian", "callback", "qp"])
    ap.add_argument("--worker", choices=["laplacian", "callback", "qp"])
    ap.add_argument("--form", default="csr", choices=["csr", "stencil"])
    ap.add_argument("--nx", type=int, default=None)
    ap.add_argument("--n", type=int, default=3_333_336)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cb-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    args = ap.parse_args()
    if args.nx is None:
        args.nx = 1000 if (args.worker or args.case) == "callback" else 2048
    if args.worker:
        worker(args)
        return
    os.makedirs(args.out, exist_ok=True)
    base = [sys.executable, os.path.abspath(__file__), "--worker", args.case, "--nx", str(args.nx), "--n", str(args.n),
            "--steps", str(args.steps), "--cb-steps", str(args.cb_steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
    env = dict(os.environ)
    env.pop("BZ_SPQ_FUSED", None)
    env.pop("BZ_SPMV_L", None)
    if args.case == "laplacian":
        res = {"case": "laplacian", "one_launch": child(base, dict(env, BZ_SPQ_FUSED="1"), args.limit),
               "two_launch": child(base, dict(env, BZ_SPQ_FUSED="0"), args.limit),
               "stencil": child(base + ["--form", "stencil"], env, args.limit)}
        a, b, s = (res[k]["run"] for k in ("one_launch", "two_launch", "stencil"))
        res["one_over_two_launch"] = a["it_per_s_median"] / b["it_per_s_median"]
        res["one_launch_over_stencil"] = a["it_per_s_median"] / s["it_per_s_median"]
        res["spread_it_per_s"] = max(a["it_per_s_max"] - a["it_per_s_min"], b["it_per_s_max"] - b["it_per_s_min"])
    else:
        res = child(base, env, args.limit)
    rocprof = shutil.which("rocprofv3")
    if args.case == "qp":
        if rocprof:
            d = os.path.join(args.out, "rocprof_sparse_qp")
            shutil.rmtree(d, ignore_errors=True)
            short = list(base)
            short[short.index("--steps") + 1] = "40"
            short[short.index("--repeats") + 1] = "1"
            child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + short, env, args.limit)
            ks = kernel_stats(d, ("k_spmv_q", "k_spmv_yupd", "k_spmv_t_finish", "k_spmv_fold"))
            shutil.rmtree(d, ignore_errors=True)
            for k, m in zip(("k_spmv_q", "k_spmv_yupd", "k_spmv_t_finish"), res["model"]):
                if k in ks:
                    ks[k]["bytes"] = m["bytes"]
                    ks[k]["fraction_of_8TBs"] = m["bytes"] / (ks[k]["avg_us"] * 1e-6) / HBM_PEAK
            res["per_kernel"] = ks
        else:
            res["per_kernel"] = "rocprofv3 not found: category 9 (the three kernels together) only"
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, f"sparse_qp_{args.case}.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
