#!/usr/bin/env python
"""Measure the elastic net g (BZ_G_ELASTIC_NET, the new arm of prox_elem) on the MI355X.  bench.py is not involved.

    python tools/bench_elastic_net.py

1. The kernel: k_fbstep with g = ElasticNet as a number pair and with weights, beside g = NormL1(array) on the SAME vectors
   (the same run-time form without the division and the second product), n = 10^7, fp64.  f = DiagQuadratic, c = Identity,
   D = Box (synth.l1_quadratic) with fuse = 0, so that every problem runs the kernel chain and every iteration launches the
   forward-backward step on x, grad L, z and res (and, with a vector, the weights).  Kernel time from the library's own HIP
   events (category 3, fb_step); `repeats` runs of `steps` launches each, the median and the range; the share of the HBM
   peak by the library's byte model.
2. The solve: synth.sparse_logistic(m = 5 * 10^6, n = 10^7, k = 5) with g = ElasticNet.glmnet(0.1, 0.5) beside g = NormL1(0.1)
   — the run of tools/bench_sparse_logistic.py — iterations per second (warm-up, then `repeats` timed calls of bz_panoc_steps).

Prints ONE JSON line and writes it to <out>/elastic_net.json.  Every GPU step is a child process under a time limit of its
own; the first one that fails ends the run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_group_lasso import ragged_case as repeated_fb_kernel         # noqa: E402
from tools.bench_sparse import child as run_child, run_problem                # noqa: E402
from tools.bench_sparse_logistic import commit_of_tree                       # noqa: E402


def kernel_worker(bz, args):
    n = args.n
    d = bz.synth.l1_quadratic(n, dtype=np.float64)
    lam = float(d["lam"])
    w = np.random.default_rng(0).uniform(0.0, 2.0, n)
    w[[0, n // 2, n - 1]] = 0.0
    cases = {"norm_l1_array": bz.NormL1(lam * w),
             "elastic_net_weights": bz.ElasticNet(lam, 0.5 * lam, w),
             "elastic_net_numbers": bz.ElasticNet(lam, 0.5 * lam),
             "norm_l1_number": bz.NormL1(lam)}
    res = {"n": n, "dtype": "float64", "steps": args.steps, "repeats": args.repeats, "l1": lam, "l2": 0.5 * lam}
    for name, g in cases.items():
        res[name] = repeated_fb_kernel(bz, g, d, n, args.steps, args.repeats)
    for name in ("elastic_net_weights", "elastic_net_numbers"):
        res[name + "_over_norm_l1_array"] = res[name]["avg_us_median"] / res["norm_l1_array"]["avg_us_median"]
    return res


def solve_worker(bz, args):
    dt = np.float64
    d = bz.synth.sparse_logistic(args.m, args.n, args.k, dt)
    f = bz.SparseLogistic(d["indptr"], d["indices"], d["data"], d["labels"], args.n)
    rest = (bz.IdentityFunction(), bz.FreeSet())
    res = {"m": f.m, "n": f.n, "nnz": f.nnz, "dtype": "float64", "lambda": 0.1, "alpha": 0.5}
    res["elastic_net"] = run_problem(bz, (f, bz.ElasticNet.glmnet(0.1, 0.5)) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)
    res["l1"] = run_problem(bz, (f, bz.NormL1(0.1)) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)
    res["elastic_net_over_l1_it_per_s"] = res["elastic_net"]["it_per_s_median"] / res["l1"]["it_per_s_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="kernel: the step kernel's comparison ; solve: the sparse logistic fits")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--m", type=int, default=5_000_000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-solve", action="store_true", help="the kernel comparison alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--commit", default=None, help="the commit of the measured tree, recorded with the result")
    ap.add_argument("--limit", type=int, default=600, help="seconds per child process")
    args = ap.parse_args()
    if args.worker:
        import bazinga_jl_amd as bz
        res = kernel_worker(bz, args) if args.worker == "kernel" else solve_worker(bz, args)
        print("RESULT " + json.dumps(res), flush=True)
        return
    os.makedirs(args.out, exist_ok=True)

    def cmd(kind):
        opts = {"--n": args.n, "--m": args.m, "--k": args.k, "--steps": args.steps, "--warmup": args.warmup, "--repeats": args.repeats}
        return [sys.executable, os.path.abspath(__file__), "--worker", kind] + [str(v) for kv in opts.items() for v in kv]
    env = dict(os.environ)
    res = {"commit": args.commit or commit_of_tree(), "kernel": run_child(cmd("kernel"), env, args.limit)}
    sys.stderr.write("[bench_elastic_net] kernel done\n")
    sys.stderr.flush()
    if not args.no_solve:
        res["solve"] = run_child(cmd("solve"), env, args.limit)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, "elastic_net.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
