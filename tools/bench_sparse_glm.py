#!/usr/bin/env python
"""Measure the sparse GLM f (BZ_F_SPARSE_GLM) on the MI355X.  bench.py is not involved.

    python tools/bench_sparse_glm.py --case losses     # synth.sparse_glm(m = 5e6, n = 1e7, k = 5), g = NormL1, c = Identity, D = Free,
                                                       # fp64: it/s per loss (Huber, squared hinge, Poisson, Huber with a weight
                                                       # vector and the scale 1 / m) beside kinds 7 and 8 on the same matrix, and
                                                       # each k_spmv_glm_r against k_spmv_ls_r and k_spmv_logit_r
    python tools/bench_sparse_glm.py --case callback   # sparse_glm(5e5, 1e6, 5, "huber"): lowered kind against the callback kinds
    python tools/bench_sparse_glm.py --case intercept  # the Lasso of `losses` (kind 7) with one more column of ones: g = NormL1 with
                                                       # a vector lambda that is zero at that column, beside the same matrix with
                                                       # the number lambda; it/s of both, and every kernel's time from a
                                                       # rocprofv3 run of each (the prox launches: one more stream of n elements)

Each case prints ONE JSON line and writes it to <out>/sparse_glm_<case>.json.  Per run: warm-up steps, then `repeats` timed calls
of bz_panoc_steps(K): median, minimum and maximum it/s.  The row kernels share the profile's category 9, so the per-kernel times
come from further runs of the same worker under `rocprofv3 --kernel-trace --stats` (skipped with a note where that tool is
missing); the weighted run has a process of its own there, because its kernel has the name of the unweighted one.  Every GPU
step is a child process under a time limit of its own; the first one that fails ends the run."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_sparse import HBM_PEAK, run_problem                   # noqa: E402
from tools.bench_sparse import child as run_child                       # noqa: E402
from tools.bench_sparse_logistic import commit_of_tree                  # noqa: E402
from tools.bench_sparse_ls import ls_bytes                              # noqa: E402
from tools.bench_sparse_qp import HostOnly                              # noqa: E402

KINDS = ("ls", "logit", "huber", "squared_hinge", "poisson", "huber_w")
INTERCEPT = ("icpt", "icpt_vec")      # the Lasso with a column of ones: a number lambda, a vector lambda with a zero at that column
MODES = {8: "least_squares", 9: "logistic", 10: "huber", 11: "squared_hinge", 12: "poisson"}      # k_spmv_glm_r's last argument


def problem(bz, kind, m, n, k, dtype):
    rest = (bz.NormL1(0.1), bz.IdentityFunction(), bz.FreeSet())
    if kind in INTERCEPT:
        d = bz.synth.sparse_glm(m, n, k, "least_squares", dtype)
        # (one more entry per row, behind the row's own: column n, value 1)
        lens = np.diff(d["indptr"])
        indptr = (d["indptr"] + np.arange(m + 1)).astype(np.int64)
        at = indptr[1:] - 1
        indices, data = np.empty(d["indices"].shape[0] + m, np.int32), np.empty(d["data"].shape[0] + m, dtype)
        own = np.ones(indices.shape[0], bool)
        own[at] = False
        indices[own], data[own], indices[at], data[at] = d["indices"], d["data"], n, 1.0
        assert np.array_equal(np.diff(indptr), lens + 1)
        lam = np.full(n + 1, 0.1)
        lam[n] = 0.0
        g = bz.NormL1(lam if kind == "icpt_vec" else 0.1)
        return bz.SparseLeastSquares(indptr, indices, data, d["b"], n + 1), (g,) + rest[1:]
    if kind in ("ls", "logit"):
        d = bz.synth.sparse_glm(m, n, k, "least_squares" if kind == "ls" else "logistic", dtype)
        cls = bz.SparseLeastSquares if kind == "ls" else bz.SparseLogistic
        return cls(d["indptr"], d["indices"], d["data"], d["b"], n), rest
    loss = kind[:-2] if kind.endswith("_w") else kind
    d = bz.synth.sparse_glm(m, n, k, loss, dtype)
    w = (0.5 + bz.synth.uniform(11, m)).astype(dtype) if kind.endswith("_w") else None
    f = bz.SparseGLM(d["indptr"], d["indices"], d["data"], d["b"], n, loss, delta=d["delta"], weights=w, scale=1.0 / m if w is not None else 1.0)
    return f, ((bz.NormL1(0.1 / m),) + rest[1:] if w is not None else rest)


def model_bytes(f, dtype):
    """the byte model of the least-squares kind; the first launch of the GLM kind streams m more elements when its weights are
    a vector"""
    out = ls_bytes(f, dtype)
    extra = f.m * np.dtype(dtype).itemsize if getattr(f, "weights", None) is not None else 0
    out["first_launch"] = {"bytes": out["k_spmv_ls_r"]["bytes"] + extra}
    if hasattr(f, "loss"):                                   # (the GLM kind's first launch is k_spmv_glm_r, not k_spmv_ls_r)
        out[f"k_spmv_glm_r<{f.loss}>"] = dict(out.pop("k_spmv_ls_r"), bytes=out["first_launch"]["bytes"])
    elif hasattr(f, "_loss_r"):
        out["k_spmv_logit_r"] = out.pop("k_spmv_ls_r")
    return out


def kernel_stats(directory):
    """per row kernel (k_spmv_glm_r by its loss): calls, average / minimum / maximum duration (us) and the standard deviation"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "").replace("void bz::", "").replace(" ", "")
            m = re.match(r"(k_spmv_\w+)<([^<>]*)>", name)
            if not m or not row.get("Calls"):
                continue
            key = m.group(1)
            if key == "k_spmv_glm_r":
                key += "<" + MODES.get(int(m.group(2).split(",")[-1]), "?") + ">"
            a = out.setdefault(key, {"calls": 0, "total_ns": 0.0, "min_ns": float("inf"), "max_ns": 0.0, "std_ns": []})
            a["calls"] += int(row["Calls"]); a["total_ns"] += float(row.get("TotalDurationNs") or 0.0)
            a["min_ns"] = min(a["min_ns"], float(row.get("MinNs") or "inf"))
            a["max_ns"] = max(a["max_ns"], float(row.get("MaxNs") or 0.0))
            if row.get("StdDev"):
                a["std_ns"].append(float(row["StdDev"]))
    return {k: {"calls": v["calls"], "avg_us": v["total_ns"] / v["calls"] / 1e3, "min_us": v["min_ns"] / 1e3, "max_us": v["max_ns"] / 1e3,
                "std_us": max(v["std_ns"]) / 1e3 if v["std_ns"] else None} for k, v in out.items() if v["calls"]}


def all_kernel_stats(directory):
    """per kernel (template arguments dropped): calls and the average duration (us)"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = re.sub(r"<.*", "", row.get("Name", "").replace("void bz::", "").replace("bz::", "")).strip()
            if not name.startswith("k_") or not row.get("Calls"):
                continue
            a = out.setdefault(name, {"calls": 0, "total_ns": 0.0})
            a["calls"] += int(row["Calls"]); a["total_ns"] += float(row.get("TotalDurationNs") or 0.0)
    return {k: {"calls": v["calls"], "avg_us": v["total_ns"] / v["calls"] / 1e3} for k, v in out.items() if v["calls"]}


def worker(args):
    import bazinga_jl_amd as bz
    dt = np.float64
    res = {"dtype": "float64", "runs": {}}
    for kind in args.worker.split(","):
        f, rest = problem(bz, kind, args.m, args.n, args.k, dt)
        res.update(m=f.m, n=f.n, nnz=f.nnz)
        r = {"model": model_bytes(f, dt), "run": run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)}
        if args.callback:
            r["callback"] = run_problem(bz, (HostOnly(f),) + rest, f.n, f.n, dt, args.cb_steps, 3, 3, events=False)
            r["speedup"] = r["run"]["it_per_s_median"] / r["callback"]["it_per_s_median"]
        res["runs"][kind] = r
        sys.stderr.write(f"[bench_sparse_glm] {kind} done\n")
        sys.stderr.flush()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["losses", "callback", "intercept"])
    ap.add_argument("--worker", default=None, help="comma-separated kinds of " + ", ".join(KINDS + INTERCEPT))
    ap.add_argument("--callback", type=int, default=0)
    ap.add_argument("--m", type=int, default=None)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cb-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--commit", default=None, help="the commit of the measured tree, recorded with the result")
    ap.add_argument("--limit", type=int, default=600, help="seconds per child process")
    args = ap.parse_args()
    small = args.case == "callback" or args.callback
    if args.n is None:
        args.n = 1_000_000 if small else 10_000_000
    if args.m is None:
        args.m = args.n // 2
    if args.worker:
        worker(args)
        return
    os.makedirs(args.out, exist_ok=True)

    def cmd(kinds, **over):
        opts = {"--m": args.m, "--n": args.n, "--k": args.k, "--steps": args.steps, "--cb-steps": args.cb_steps, "--warmup": args.warmup,
                "--repeats": args.repeats}
        opts.update(over)
        return [sys.executable, os.path.abspath(__file__), "--worker", kinds] + [str(v) for kv in opts.items() for v in kv]

    def child(command, environment, what):      # (progress on stderr: a case is several minutes of child processes)
        out = run_child(command, environment, args.limit)
        sys.stderr.write(f"[bench_sparse_glm] {what} done\n")
        sys.stderr.flush()
        return out
    env = dict(os.environ)
    env.pop("BZ_SPLS_FUSED", None)
    env.pop("BZ_SPMV_L", None)
    if args.case == "losses":
        res = child(cmd(",".join(KINDS)), env, "it/s of " + ", ".join(KINDS))
        res.update(case="losses", commit=args.commit or commit_of_tree())
        res["it_per_s_median"] = {k: v["run"]["it_per_s_median"] for k, v in res["runs"].items()}
        rocprof = shutil.which("rocprofv3")
        if rocprof:
            res["per_kernel"] = {}
            for name, kinds in (("unweighted", ",".join(KINDS[:5])), ("huber_w", "huber_w")):
                d = os.path.join(args.out, "rocprof_sparse_glm_" + name)
                shutil.rmtree(d, ignore_errors=True)
                child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd(kinds, **{"--steps": 40, "--repeats": 1}),
                      env, "rocprofv3 " + name)
                ks = kernel_stats(d)
                shutil.rmtree(d, ignore_errors=True)
                res["per_kernel"][name] = ks
            un, first = res["per_kernel"]["unweighted"], res["runs"]["huber"]["model"]["first_launch"]["bytes"]
            ls, lg = un.get("k_spmv_ls_r"), un.get("k_spmv_logit_r")
            if ls and lg:
                res["glm_r_against_the_existing_kernels"] = {
                    k: {"avg_us": v["avg_us"], "minus_ls_r_us": v["avg_us"] - ls["avg_us"], "minus_logit_r_us": v["avg_us"] - lg["avg_us"],
                        "fraction_of_8TBs": first / (v["avg_us"] * 1e-6) / HBM_PEAK}
                    for k, v in un.items() if k.startswith("k_spmv_glm_r")}
                res["ls_r_spread_us"], res["ls_r_std_us"] = ls["max_us"] - ls["min_us"], ls["std_us"]
            hw, hu = res["per_kernel"]["huber_w"].get("k_spmv_glm_r<huber>"), un.get("k_spmv_glm_r<huber>")
            if hw and hu:
                res["weight_vector_cost_us"] = hw["avg_us"] - hu["avg_us"]
        else:
            res["per_kernel"] = "rocprofv3 not found: category 9 (the row kernels together) only"
    elif args.case == "intercept":
        res = child(cmd(",".join(INTERCEPT)), env, "it/s of " + ", ".join(INTERCEPT))
        res.update(case="intercept", commit=args.commit or commit_of_tree())
        res["it_per_s_median"] = {k: v["run"]["it_per_s_median"] for k, v in res["runs"].items()}
        res["it_per_s_vector_over_number"] = res["it_per_s_median"]["icpt_vec"] / res["it_per_s_median"]["icpt"]
        # the byte model: one more stream of n elements in every launch that evaluates the prox, nothing in the row kernels
        res["model_extra_bytes_per_prox_launch"] = res["n"] * 8
        rocprof = shutil.which("rocprofv3")
        if rocprof:
            res["per_kernel"] = {}
            for kind in INTERCEPT:      # (a process each: the kernels have the same names)
                d = os.path.join(args.out, "rocprof_sparse_glm_" + kind)
                shutil.rmtree(d, ignore_errors=True)
                child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd(kind, **{"--steps": 40, "--repeats": 1}),
                      env, "rocprofv3 " + kind)
                res["per_kernel"][kind] = all_kernel_stats(d)
                shutil.rmtree(d, ignore_errors=True)
            a, b = res["per_kernel"]["icpt"], res["per_kernel"]["icpt_vec"]
            res["vector_minus_number_us"] = {k: b[k]["avg_us"] - a[k]["avg_us"] for k in sorted(set(a) & set(b))}
            # (what the extra stream would cost at the HBM peak)
            res["model_extra_us_at_8TBs"] = res["model_extra_bytes_per_prox_launch"] / HBM_PEAK * 1e6
        else:
            res["per_kernel"] = "rocprofv3 not found"
    else:
        res = child(cmd("huber", **{"--callback": 1}), env, "lowered against callbacks")
        res.update(case="callback", commit=args.commit or commit_of_tree(), speedup=res["runs"]["huber"]["speedup"])
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, f"sparse_glm_{args.case}.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
