#!/usr/bin/env python
"""Measure the sparse multinomial f (BZ_F_SPARSE_MULTINOMIAL) on the MI355X.  bench.py is not involved.

    python tools/bench_sparse_multinomial.py      # synth.sparse_multinomial(m = 5e6, n_f = 1.25e6, K, k = 5) at K = 2, 8, 32
                                                  # (n = n_f K: 10^7 at K = 8), g = NormL1, c = Identity, D = Free, fp64, beside
                                                  # the binary SparseLogistic on the SAME matrix (n = n_f)

Prints ONE JSON line and writes it to <out>/sparse_multinomial.json: per run the iterations per second (warm-up steps, then
`repeats` timed calls of bz_panoc_steps(K): median, minimum and maximum), and, from further runs of the same worker under
`rocprofv3 --kernel-trace --stats` (skipped with a note where that tool is missing), each row kernel's time with its share of
the HBM peak by the byte model, and the time of k_spmm_softmax_r beside k_spmv_logit_r: the cost of a K-class launch in binary
launches on the same matrix, with the spread of the repeats.  Every GPU step is a child process under a time limit of its own;
the first one that fails ends the run.

(The first step size is given, gamma = 1 with adaptive = True: PANOCplus estimates it from grad L(x0 + 1) - grad L(x0), and adding
one number to all K classes of a feature leaves the softmax unchanged, so with D = Free that estimate is 0.)"""
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

from tools.bench_sparse import HBM_PEAK, plan, run_problem, timed_steps      # noqa: E402
from tools.bench_sparse import child as run_child                            # noqa: E402
from tools.bench_sparse_logistic import commit_of_tree                       # noqa: E402
from tools.bench_sparse_ls import ls_bytes                                   # noqa: E402

CLASSES = (2, 8, 32)


def plan_k(indptr, nnz, K):
    """bz_spmm.h's plan: the segment rule of the scalar kernels, lanes per class under KP * L <= 64"""
    _, nv, seg = plan(indptr, nnz)
    kp = 2
    while kp < K:
        kp *= 2
    mean = nnz / nv if nv else 0.0
    L = 1
    while kp * L * 2 <= 64 and mean > 4.0 * L:
        L *= 2
    return L, nv, seg


def mn_bytes(f, dtype):
    """the byte model of the three K-wide passes: the matrix once per pass (both CSR arrays, the virtual row pointers and the
    tables of a cut matrix), one read of the K-wide gathered vector, and per row the label, the weight where it is a vector
    and K of R (k_spmm_softmax_r) / per element x, mu, mu*y and the gradient (k_spmm_t_algrad) / the product (k_spmm_t)"""
    sz, K = np.dtype(dtype).itemsize, f.n_classes
    tptr = np.concatenate(([0], np.cumsum(np.bincount(f.indices, minlength=f.n_features)))).astype(np.int64)
    out = {}
    for name, ptr, gathered, vec in (("k_spmm_softmax_r", f.indptr, f.n, (1 + K + (f.weights is not None)) * f.m),
                                     ("k_spmm_t_algrad", tptr, f.m * K, 4 * f.n), ("k_spmm_t", tptr, f.m * K, f.n)):
        L, nv, seg = plan_k(ptr, f.nnz, K)
        out[name] = {"L": L, "segmented": seg, "bytes": f.nnz * (sz + 4) + (nv + 1) * 8 + (nv * 8 if seg else 0) + (gathered + vec) * sz}
    return out


def kernel_stats(directory):
    """per row kernel (template arguments dropped): calls, average / minimum / maximum duration (us), the standard deviation"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            m = re.match(r"(k_sp(?:mv|mm)_\w+)<", row.get("Name", "").replace("void bz::", "").replace(" ", ""))
            if not m or not row.get("Calls"):
                continue
            a = out.setdefault(m.group(1), {"calls": 0, "total_ns": 0.0, "min_ns": float("inf"), "max_ns": 0.0, "std_ns": []})
            a["calls"] += int(row["Calls"]); a["total_ns"] += float(row.get("TotalDurationNs") or 0.0)
            a["min_ns"] = min(a["min_ns"], float(row.get("MinNs") or "inf"))
            a["max_ns"] = max(a["max_ns"], float(row.get("MaxNs") or 0.0))
            if row.get("StdDev"):
                a["std_ns"].append(float(row["StdDev"]))
    return {k: {"calls": v["calls"], "avg_us": v["total_ns"] / v["calls"] / 1e3, "min_us": v["min_ns"] / 1e3, "max_us": v["max_ns"] / 1e3,
                "std_us": max(v["std_ns"]) / 1e3 if v["std_ns"] else None} for k, v in out.items() if v["calls"]}


def run_multinomial(bz, f, dtype, K, warmup, repeats):
    n = f.n
    prob = bz.Problem(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
    prob.set_multipliers(np.full(n, 0.1, dtype), np.zeros(n, dtype))
    opts = bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(dtype).eps), gamma=1.0, adaptive=True).c_opts()
    prob.panoc_begin(opts, np.zeros(n, dtype))
    out = timed_steps(prob, K, warmup, repeats)
    prob.profile_reset()
    prob.profile_enable(1 << 9)
    prob.panoc_steps(min(K, 50))
    g = prob.profile2()["gemv"]
    out["category9"] = {"launches": g["launches"], "bytes": g["bytes"], "timed_launches": g["timed_launches"], "timed_ms": g["timed_ms"],
                        "timed_bytes": g["timed_bytes"], "form_of_last_launch": g["form"],
                        "fraction_of_8TBs": g["timed_bytes"] / (g["timed_ms"] * 1e-3) / HBM_PEAK if g["timed_ms"] else None}
    prob.profile_enable(False)
    st = prob.panoc_stats()
    out["n_grad"], out["n_backtracks"], out["n_gamma_halvings"] = st.n_grad, st.n_backtracks, st.n_gamma_halvings
    prob.close()
    return out


def worker(args):
    import bazinga_jl_amd as bz
    dt = np.float64
    res = {"dtype": "float64", "m": args.m, "n_f": args.nf, "k": args.k, "runs": {}}
    for kind in args.worker.split(","):
        if kind == "logit":                                   # the yardstick: the binary kind on the same matrix
            d = bz.synth.sparse_logistic(args.m, args.nf, args.k, dt)
            f = bz.SparseLogistic(d["indptr"], d["indices"], d["data"], d["labels"], args.nf)
            rest = (bz.NormL1(0.1), bz.IdentityFunction(), bz.FreeSet())
            model = ls_bytes(f, dt)
            model["k_spmv_logit_r"] = model.pop("k_spmv_ls_r")
            r = {"n": f.n, "model": model, "run": run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)}
        else:
            K = int(kind[2:])
            d = bz.synth.sparse_multinomial(args.m, args.nf, K, args.k, dt)
            f = bz.SparseMultinomial(d["indptr"], d["indices"], d["data"], d["labels"], args.nf, K)
            r = {"n": f.n, "K": K, "model": mn_bytes(f, dt), "run": run_multinomial(bz, f, dt, args.steps, args.warmup, args.repeats)}
        res["nnz"] = f.nnz
        res["runs"][kind] = r
        sys.stderr.write(f"[bench_sparse_multinomial] {kind} done\n")
        sys.stderr.flush()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="comma-separated kinds of logit, mn2, mn8, mn32 (mn<K>)")
    ap.add_argument("--m", type=int, default=5_000_000)
    ap.add_argument("--nf", type=int, default=1_250_000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--classes", default=",".join(str(c) for c in CLASSES))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--commit", default=None, help="the commit of the measured tree, recorded with the result")
    ap.add_argument("--limit", type=int, default=600, help="seconds per child process")
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return
    os.makedirs(args.out, exist_ok=True)
    kinds = ["logit"] + ["mn" + c for c in args.classes.split(",")]

    def cmd(kind, **over):
        opts = {"--m": args.m, "--nf": args.nf, "--k": args.k, "--steps": args.steps, "--warmup": args.warmup, "--repeats": args.repeats}
        opts.update(over)
        return [sys.executable, os.path.abspath(__file__), "--worker", kind] + [str(v) for kv in opts.items() for v in kv]

    def child(command, environment, what):
        out = run_child(command, environment, args.limit)
        sys.stderr.write(f"[bench_sparse_multinomial] {what} done\n")
        sys.stderr.flush()
        return out
    env = dict(os.environ)
    env.pop("BZ_SPLS_FUSED", None)
    env.pop("BZ_SPMV_L", None)
    res = {"commit": args.commit or commit_of_tree(), "runs": {}}
    for kind in kinds:                                          # (a process each: the K = 32 problem holds 40 vectors of 4e7)
        r = child(cmd(kind), env, "it/s of " + kind)
        res.update({k: v for k, v in r.items() if k != "runs"})
        res["runs"].update(r["runs"])
    res["it_per_s_median"] = {k: v["run"]["it_per_s_median"] for k, v in res["runs"].items()}
    rocprof = shutil.which("rocprofv3")
    if rocprof:
        res["per_kernel"] = {}
        for kind in kinds:                                      # (a process each: the kernels of different K share their names)
            d = os.path.join(args.out, "rocprof_sparse_multinomial_" + kind)
            shutil.rmtree(d, ignore_errors=True)
            child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd(kind, **{"--steps": 40, "--repeats": 1}),
                  env, "rocprofv3 " + kind)
            ks = kernel_stats(d)
            shutil.rmtree(d, ignore_errors=True)
            for name, v in ks.items():
                b = res["runs"][kind]["model"].get(name)
                if b:
                    v["fraction_of_8TBs"] = b["bytes"] / (v["avg_us"] * 1e-6) / HBM_PEAK
            res["per_kernel"][kind] = ks
        lg = res["per_kernel"]["logit"].get("k_spmv_logit_r")
        if lg:
            res["softmax_r_against_logit_r"] = {}
            for kind in kinds[1:]:
                sm = res["per_kernel"][kind].get("k_spmm_softmax_r")
                if sm:
                    res["softmax_r_against_logit_r"][kind] = {
                        "K": res["runs"][kind]["K"], "softmax_r_us": sm["avg_us"], "logit_r_us": lg["avg_us"], "ratio": sm["avg_us"] / lg["avg_us"],
                        "ratio_min": sm["min_us"] / lg["max_us"], "ratio_max": sm["max_us"] / lg["min_us"],
                        "binary_launches_per_class": sm["avg_us"] / lg["avg_us"] / res["runs"][kind]["K"]}
    else:
        res["per_kernel"] = "rocprofv3 not found: category 9 (the row kernels together) only"
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, "sparse_multinomial.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
