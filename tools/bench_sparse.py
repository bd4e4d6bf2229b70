#!/usr/bin/env python
"""Measure the sparse affine constraint (BZ_C_SPARSE_AFFINE) on the MI355X.  bench.py is not involved.

    python tools/bench_sparse.py --case obstacle          # synth.obstacle_1d, N = 3.3e6 (n ~ 1e7), fp64
    python tools/bench_sparse.py --case callback          # obstacle_1d at n ~ 1e6: lowered kind against the callback kinds
    python tools/bench_sparse.py --case cfg4              # basis_pursuit's matrix as CSR against the DenseAffine kind, fp32

Each case prints ONE JSON line and writes it to <out>/sparse_<case>.json.  Per case: warm-up steps, then `repeats` timed
calls of bz_panoc_steps(K) (the call returns when its results are on the host): median, minimum and maximum it/s.  The
two row kernels are timed by HIP events on their own dispatches (category 9); the two share that category, so the
per-kernel times come from a second run of the same worker under `rocprofv3 --kernel-trace --stats` (skipped with a note
in the output where that tool is missing).  Every GPU step is a child process under a time limit of its own; the first
one that fails ends the run."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # bytes / s


def plan(indptr, nnz):
    """segment length, virtual rows, lanes per row"""
    S = max(512, ((nnz // (2048 * 4) // 4 + 63) // 64) * 64)
    lens = np.diff(indptr)
    nv = int(np.where(lens > S, -(-lens // S), 1).sum())
    seg = bool(np.any(lens > S))
    mean = nnz / nv if nv else 0.0
    L = 1
    while L < 64 and mean > 4.0 * L:
        L *= 2
    return L, nv, seg


def pass_bytes(c, dtype, per_row_y, per_row_x):
    """bytes of k_spmv_yupd and k_spmv_t_finish for the matrix of SparseAffine c (DESIGN 4's model)"""
    sz = np.dtype(dtype).itemsize
    tptr = np.concatenate(([0], np.cumsum(np.bincount(c.indices, minlength=c.n)))).astype(np.int64)
    out = []
    for ptr, gathered, vecs, rows in ((c.indptr, c.n, per_row_y, c.ny), (tptr, c.ny, per_row_x, c.n)):
        L, nv, seg = plan(ptr, c.nnz)
        out.append({"L": L, "segmented": seg,
                    "bytes": c.nnz * (sz + 4) + (nv + 1) * 8 + (nv * 8 if seg else 0) + gathered * sz + vecs * rows * sz})
    return out


class HostOnly:
    """hides the type of a lowered oracle: the problem then runs through the callback kinds (what the library did with a
    sparse c before this kind existed), evaluating the same CSR arrays on the host with numpy"""

    def __init__(self, c):
        self.eval, self.jtprod = c.eval, c.jtprod


def timed_steps(prob, K, warmup, repeats):
    prob.panoc_steps(warmup)
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        prob.panoc_steps(K)
        rates.append(K / (time.perf_counter() - t0))
    return {"K": K, "warmup": warmup, "repeats": repeats, "it_per_s_median": statistics.median(rates),
            "it_per_s_min": min(rates), "it_per_s_max": max(rates)}


def run_problem(bz, dev, n, ny, dtype, K, warmup, repeats, events=True):
    prob = bz.Problem(*dev, n, ny, dtype)
    prob.set_multipliers(np.full(ny, 0.1, dtype), np.zeros(ny, dtype))
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(dtype).eps)).c_opts(), np.zeros(n, dtype))
    out = timed_steps(prob, K, warmup, repeats)
    if events:
        prob.profile_reset()
        prob.profile_enable(1 << 9)
        prob.panoc_steps(min(K, 50))
        g = prob.profile2()["gemv"]
        out["category9"] = {"launches": g["launches"], "bytes": g["bytes"], "timed_launches": g["timed_launches"],
                            "timed_ms": g["timed_ms"], "timed_bytes": g["timed_bytes"], "form_of_last_launch": g["form"],
                            "fraction_of_8TBs": g["timed_bytes"] / (g["timed_ms"] * 1e-3) / HBM_PEAK if g["timed_ms"] else None}
        prob.profile_enable(False)
    st = prob.panoc_stats()
    out["n_grad"], out["n_backtracks"], out["n_gamma_halvings"] = st.n_grad, st.n_backtracks, st.n_gamma_halvings
    prob.close()
    return out


def obstacle(bz, N, dtype):
    d = bz.synth.obstacle_1d(N, dtype)
    c = bz.SparseAffine(d["indptr"], d["indices"], d["data"], d["b"], d["n"])
    return d, c, (bz.DiagQuadratic(d["q"], d["fb"]), bz.NormL1Nonneg(0.1), c, bz.ZeroSet())


def worker(args):
    import bazinga_jl_amd as bz
    res = {"case": args.worker, "BZ_SPMV_L": os.environ.get("BZ_SPMV_L")}
    if args.worker == "obstacle":
        d, c, dev = obstacle(bz, args.N, np.float64)
        res.update(n=c.n, ny=c.ny, nnz=c.nnz, dtype="float64")
        res["model"] = pass_bytes(c, np.float64, 4, 4)      # b, mu, mu*y, yhat | x, q, b, grad
        res["lowered"] = run_problem(bz, dev, c.n, c.ny, np.float64, args.steps, args.warmup, args.repeats)
    elif args.worker == "callback":
        d, c, dev = obstacle(bz, args.N, np.float64)
        res.update(n=c.n, ny=c.ny, nnz=c.nnz, dtype="float64")
        res["lowered"] = run_problem(bz, dev, c.n, c.ny, np.float64, args.steps, args.warmup, args.repeats)
        res["callback"] = run_problem(bz, dev[:2] + (HostOnly(c),) + dev[3:], c.n, c.ny, np.float64, args.cb_steps, 3, 3, events=False)
        res["speedup"] = res["lowered"]["it_per_s_median"] / res["callback"]["it_per_s_median"]
    elif args.worker == "cfg4":
        ny, n = args.shape
        d = bz.synth.basis_pursuit(ny, n, dtype=np.float32, density=0.01)
        c = bz.SparseAffine.from_dense(d["A"], d["b"])
        res.update(n=n, ny=ny, nnz=c.nnz, dtype="float32")
        res["model"] = pass_bytes(c, np.float32, 4, 1)      # f = Zero: the gradient alone on the x side
        g = (bz.Zero(), bz.NormL1(1.0))
        res["sparse"] = run_problem(bz, g + (c, bz.ZeroSet()), n, ny, np.float32, args.steps, args.warmup, args.repeats)
        res["dense"] = run_problem(bz, g + (bz.DenseAffine(d["A"], d["b"]), bz.ZeroSet()), n, ny, np.float32, args.steps,
                                   args.warmup, args.repeats)
    print("RESULT " + json.dumps(res), flush=True)


def child(cmd, env, limit):
    p = subprocess.run(cmd, env=env, cwd=ROOT, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit(f"{' '.join(cmd[:6])} ... ended with status {p.returncode}: nothing more is started")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit("the worker printed no result")


def kernel_stats(directory):
    """average duration (us) of the two row kernels from rocprofv3's kernel statistics"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            for k in ("k_spmv_yupd", "k_spmv_t_finish", "k_spmv_fold"):
                if k in name and row.get("Calls"):
                    calls = int(row["Calls"])
                    tot = float(row.get("TotalDurationNs") or 0.0)
                    a = out.setdefault(k, {"calls": 0, "total_ns": 0.0})
                    a["calls"] += calls; a["total_ns"] += tot
    return {k: {"calls": v["calls"], "avg_us": v["total_ns"] / v["calls"] / 1e3} for k, v in out.items() if v["calls"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["obstacle", "callback", "cfg4"])
    ap.add_argument("--worker", choices=["obstacle", "callback", "cfg4"])
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--shape", type=int, nargs=2, default=[4096, 16384])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cb-steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    args = ap.parse_args()
    if args.N is None:
        args.N = 333_334 if (args.worker or args.case) == "callback" else 3_300_000
    if args.worker:
        worker(args)
        return
    os.makedirs(args.out, exist_ok=True)
    base = [sys.executable, os.path.abspath(__file__), "--worker", args.case, "--N", str(args.N), "--shape", *map(str, args.shape),
            "--steps", str(args.steps), "--cb-steps", str(args.cb_steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
    env = dict(os.environ)
    env.pop("BZ_SPMV_L", None)
    res = child(base, env, args.limit)
    rocprof = shutil.which("rocprofv3")
    if args.case in ("obstacle", "cfg4"):
        runs = [None] if args.case == "cfg4" else [None, 1, 2, 4]      # the chosen L, then both passes forced to 1, 2, 4 lanes
        res["kernels"] = []
        for L in runs:
            e = dict(env)
            if L:
                e["BZ_SPMV_L"] = str(L)
            entry = {"BZ_SPMV_L": L}
            if L:
                entry["it_per_s_median"] = child(base, e, args.limit)[("lowered" if args.case == "obstacle" else "sparse")]["it_per_s_median"]
            if rocprof:
                d = os.path.join(args.out, f"rocprof_sparse_{args.case}_{L or 'chosen'}")
                shutil.rmtree(d, ignore_errors=True)
                short = [a for a in base]
                short[short.index("--steps") + 1] = "40"
                short[short.index("--repeats") + 1] = "1"
                child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + short, e, args.limit)
                ks = kernel_stats(d)
                if not ks:
                    entry["rocprof_files"] = [os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs][:20]
                shutil.rmtree(d, ignore_errors=True)
                for k, m in zip(("k_spmv_yupd", "k_spmv_t_finish"), res["model"]):
                    if k in ks:
                        ks[k]["bytes"] = m["bytes"]
                        ks[k]["fraction_of_8TBs"] = m["bytes"] / (ks[k]["avg_us"] * 1e-6) / HBM_PEAK
                entry["per_kernel"] = ks
            else:
                entry["per_kernel"] = "rocprofv3 not found: category 9 (both kernels together) only"
            res["kernels"].append(entry)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, f"sparse_{args.case}.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
