#!/usr/bin/env python
"""Measure the sparse logistic f (BZ_F_SPARSE_LOGISTIC) on the MI355X.  bench.py is not involved.

    python tools/bench_sparse_logistic.py --case logit      # synth.sparse_logistic(m = 5e6, n = 1e7, k = 5), g = NormL1, c = Identity,
                                                            # D = Free, fp64: the two-launch form against BZ_SPLS_FUSED=0, and
                                                            # k_spmv_logit_r against k_spmv_ls_r on the same matrix (the labels
                                                            # as the b of a SparseLeastSquares), both by the byte model
    python tools/bench_sparse_logistic.py --case callback   # sparse_logistic(5e5, 1e6, 5): lowered kind against the callback kinds

Each case prints ONE JSON line and writes it to <out>/sparse_logit_<case>.json.  Per run: warm-up steps, then `repeats` timed
calls of bz_panoc_steps(K) (the call returns when its results are on the host): median, minimum and maximum it/s.  The row
kernels share the profile's category 9, so the per-kernel times (average, minimum, maximum and standard deviation over the
dispatches) come from further runs of the same workers under `rocprofv3 --kernel-trace --stats` (skipped with a note where that
tool is missing).  Every GPU step is a child process under a time limit of its own; the first one that fails ends the run."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_sparse import HBM_PEAK, run_problem                   # noqa: E402
from tools.bench_sparse import child as run_child                       # noqa: E402
from tools.bench_sparse_ls import ls_bytes                              # noqa: E402
from tools.bench_sparse_qp import HostOnly                              # noqa: E402

KERNELS = ("k_spmv_logit_r", "k_spmv_ls_r", "k_spmv_ls_t_algrad", "k_spmv_ls_t", "k_spmv_fold")


def problem(bz, kind, m, n, k, dtype):
    d = bz.synth.sparse_logistic(m, n, k, dtype)
    cls = bz.SparseLogistic if kind != "ls" else bz.SparseLeastSquares
    return cls(d["indptr"], d["indices"], d["data"], d["labels"], n), (bz.NormL1(0.1), bz.IdentityFunction(), bz.FreeSet())


def model_bytes(f, dtype):
    """the byte model of the least-squares kind: the logistic row kernel streams what k_spmv_ls_r streams (per row the label
    and r)"""
    out = ls_bytes(f, dtype)
    out["k_spmv_logit_r"] = out["k_spmv_ls_r"]
    return out


def kernel_stats(directory):
    """per kernel: calls, average / minimum / maximum duration (us) and, where the tool gives it, the standard deviation"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "").replace("void bz::", "").replace(" ", "")
            for k in KERNELS:
                if name.startswith(k + "<") and row.get("Calls"):
                    a = out.setdefault(k, {"calls": 0, "total_ns": 0.0, "min_ns": float("inf"), "max_ns": 0.0, "std_ns": []})
                    a["calls"] += int(row["Calls"]); a["total_ns"] += float(row.get("TotalDurationNs") or 0.0)
                    a["min_ns"] = min(a["min_ns"], float(row.get("MinNs") or "inf"))
                    a["max_ns"] = max(a["max_ns"], float(row.get("MaxNs") or 0.0))
                    if row.get("StdDev"):
                        a["std_ns"].append(float(row["StdDev"]))
    return {k: {"calls": v["calls"], "avg_us": v["total_ns"] / v["calls"] / 1e3, "min_us": v["min_ns"] / 1e3, "max_us": v["max_ns"] / 1e3,
                "std_us": max(v["std_ns"]) / 1e3 if v["std_ns"] else None} for k, v in out.items() if v["calls"]}


def worker(args):
    import bazinga_jl_amd as bz
    dt = np.float64
    res = {"case": args.worker, "BZ_SPLS_FUSED": os.environ.get("BZ_SPLS_FUSED"), "dtype": "float64"}
    f, rest = problem(bz, args.worker, args.m, args.n, args.k, dt)
    res.update(m=f.m, n=f.n, nnz=f.nnz)
    if args.worker in ("logit", "ls"):
        res["model"] = model_bytes(f, dt)
        res["run"] = run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)
    else:
        res["lowered"] = run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)
        res["callback"] = run_problem(bz, (HostOnly(f),) + rest, f.n, f.n, dt, args.cb_steps, 3, 3, events=False)
        res["speedup"] = res["lowered"]["it_per_s_median"] / res["callback"]["it_per_s_median"]
    print("RESULT " + json.dumps(res), flush=True)


def commit_of_tree():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        return (head.stdout.strip() + ("+changes" if dirty.stdout.strip() else "")) if head.returncode == 0 else None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["logit", "callback"])
    ap.add_argument("--worker", choices=["logit", "ls", "callback"])
    ap.add_argument("--m", type=int, default=None)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cb-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--commit", default=None, help="the commit of the measured tree, recorded with the result")
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

    def cmd(kind, **over):
        opts = {"--m": args.m, "--n": args.n, "--k": args.k, "--steps": args.steps, "--cb-steps": args.cb_steps, "--warmup": args.warmup,
                "--repeats": args.repeats}
        opts.update(over)
        return [sys.executable, os.path.abspath(__file__), "--worker", kind] + [str(v) for kv in opts.items() for v in kv]

    def child(command, environment, limit, what=None):      # (progress on stderr: a case is several minutes of child processes)
        out = run_child(command, environment, limit)
        sys.stderr.write(f"[bench_sparse_logistic] {what or command[3]} done\n")
        sys.stderr.flush()
        return out
    env = dict(os.environ)
    env.pop("BZ_SPLS_FUSED", None)
    env.pop("BZ_SPMV_L", None)
    if args.case == "logit":
        res = {"case": "logit", "commit": args.commit or commit_of_tree(),
               "two_launch": child(cmd("logit"), dict(env, BZ_SPLS_FUSED="1"), args.limit),
               "three_launch": child(cmd("logit"), dict(env, BZ_SPLS_FUSED="0"), args.limit),
               "least_squares_same_matrix": child(cmd("ls"), dict(env, BZ_SPLS_FUSED="1"), args.limit)}
        a, b = res["two_launch"]["run"], res["three_launch"]["run"]
        res["two_over_three_launch"] = a["it_per_s_median"] / b["it_per_s_median"]
        res["spread_it_per_s"] = max(a["it_per_s_max"] - a["it_per_s_min"], b["it_per_s_max"] - b["it_per_s_min"])
        rocprof = shutil.which("rocprofv3")
        if rocprof:
            res["per_kernel"] = {}
            for kind in ("logit", "ls"):
                d = os.path.join(args.out, "rocprof_sparse_logit_" + kind)
                shutil.rmtree(d, ignore_errors=True)
                child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd(kind, **{"--steps": 40, "--repeats": 1}),
                      dict(env, BZ_SPLS_FUSED="1"), args.limit, what="rocprofv3 " + kind)
                ks = kernel_stats(d)
                shutil.rmtree(d, ignore_errors=True)
                for k, m in res["two_launch"]["model"].items():
                    if k in ks:
                        ks[k]["bytes"] = m["bytes"]
                        ks[k]["fraction_of_8TBs"] = m["bytes"] / (ks[k]["avg_us"] * 1e-6) / HBM_PEAK
                res["per_kernel"][kind] = ks
            lg, ls = res["per_kernel"]["logit"].get("k_spmv_logit_r"), res["per_kernel"]["ls"].get("k_spmv_ls_r")
            if lg and ls:
                res["logit_r_over_ls_r"] = {"avg_us_ratio": lg["avg_us"] / ls["avg_us"], "avg_us_difference": lg["avg_us"] - ls["avg_us"],
                                            "ls_r_spread_us": ls["max_us"] - ls["min_us"], "ls_r_std_us": ls["std_us"]}
        else:
            res["per_kernel"] = "rocprofv3 not found: category 9 (the row kernels together) only"
    else:
        res = child(cmd("callback"), env, args.limit)
        res["commit"] = args.commit or commit_of_tree()
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, f"sparse_logit_{args.case}.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
