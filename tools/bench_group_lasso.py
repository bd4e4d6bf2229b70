#!/usr/bin/env python
"""Measure the group Lasso g (BZ_G_NORM_L21, k_fbstep_group) on the MI355X.  bench.py is not involved.

    python tools/bench_group_lasso.py

1. The kernel: k_fbstep_group beside k_fbstep with g = NormL1 on the SAME vectors, n = 10^7 (rounded down to a multiple of K),
   K in 2, 8, 32, 3, 33, fp64 and fp32.  f = DiagQuadratic, c = Identity, D = Box (synth.l1_quadratic) with fuse = 0, so that both
   problems run the kernel chain and every iteration launches the forward-backward step on x, grad L, z and res: four streams
   of n, the same bytes for both kernels.  Kernel time from the library's own HIP events (category 3, fb_step), the share of
   the HBM peak by the library's byte model.
2. The solve: synth.sparse_multinomial(m, n_f, K = 8, k = 5) with g = NormL21(0.1, 8) beside g = NormL1(0.1) — the run of
   tools/bench_sparse_multinomial.py — iterations per second (warm-up, then `repeats` timed calls of bz_panoc_steps).

3. With --ragged, instead: the group Lasso over a group pointer (BZ_G_GROUP_LASSO, k_fbstep_ragged) at n = 10^7, fp64, in one
   session — all groups of 8 beside k_fbstep_group<KP=8> on the same vectors, sizes drawn uniformly from 1 .. 16, groups of 200,
   and each of the three with l1 > 0 beside l1 = 0; `repeats` runs of `steps` launches each, the median and the range.  Written to
   <out>/group_lasso_ragged.json.

Prints ONE JSON line and writes it to <out>/group_lasso.json.  Every GPU step is a child process under a time limit of its own;
the first one that fails ends the run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_sparse import HBM_PEAK, timed_steps                         # noqa: E402
from tools.bench_sparse import child as run_child                            # noqa: E402
from tools.bench_sparse_logistic import commit_of_tree                       # noqa: E402

GROUPS = (2, 8, 32, 3, 33)


def fb_kernel(bz, g, d, n, dtype, steps):
    """the forward-backward launches of `steps` iterations of the kernel chain: time, bytes, form"""
    prob = bz.Problem(bz.DiagQuadratic(d["q"][:n], d["b"][:n]), g, bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])), n, n, dtype)
    prob.set_multipliers(np.full(n, 0.1, dtype), np.zeros(n, dtype))
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(dtype).eps), fuse=False).c_opts(), np.zeros(n, dtype))
    prob.panoc_steps(5)
    prob.profile_reset()
    prob.profile_enable(1 << 3)
    prob.panoc_steps(steps)
    r = prob.profile2()["fb_step"]
    prob.profile_enable(False)
    st = prob.panoc_stats()
    prob.close()
    us = r["timed_ms"] * 1e3 / r["timed_launches"] if r["timed_launches"] else None
    return {"form_of_last_launch": r["form"], "launches": r["timed_launches"], "avg_us": us, "bytes_per_launch": r["timed_bytes"] / max(1, r["timed_launches"]),
            "fraction_of_8TBs": r["timed_bytes"] / (r["timed_ms"] * 1e-3) / HBM_PEAK if r["timed_ms"] else None,
            "n_fused_iters": int(st.n_fused_iters)}


def ragged_case(bz, g, d, n, steps, repeats):
    """`repeats` runs of fb_kernel: the median, the range, the byte-model fraction at the median"""
    runs = [fb_kernel(bz, g, d, n, np.float64, steps) for _ in range(repeats)]
    us = sorted(r["avg_us"] for r in runs)
    med = us[len(us) // 2]
    return {"form_of_last_launch": runs[0]["form_of_last_launch"], "avg_us_median": med, "avg_us_range": [us[0], us[-1]],
            "bytes_per_launch": runs[0]["bytes_per_launch"], "fraction_of_8TBs_at_median": runs[0]["bytes_per_launch"] / (med * 1e-6) / HBM_PEAK,
            "n_fused_iters": runs[0]["n_fused_iters"]}


def ragged_worker(bz, args):
    n = args.n // 200 * 200                                 # (a multiple of 8 and of 200)
    d = bz.synth.l1_quadratic(args.n, dtype=np.float64)
    lam = float(d["lam"])
    rng = np.random.default_rng(0)
    drawn = rng.integers(1, 17, n // 8)
    drawn = drawn[:np.searchsorted(np.cumsum(drawn), n)]
    drawn = np.append(drawn, n - drawn.sum()) if drawn.sum() < n else drawn
    shapes = {"uniform8": np.full(n // 8, 8), "drawn_1_16": drawn, "uniform200": np.full(n // 200, 200)}
    res = {"n": n, "dtype": "float64", "steps": args.steps, "repeats": args.repeats, "l1": 0.25 * lam, "lambda": lam,
           "norm_l21_K8": ragged_case(bz, bz.NormL21(lam, 8), d, n, args.steps, args.repeats)}
    for name, sizes in shapes.items():
        assert sizes.sum() == n and sizes.min() >= 1
        res[name] = {"groups": int(sizes.shape[0]), "largest": int(sizes.max()),
                     "l1=0": ragged_case(bz, bz.GroupLasso.from_sizes(lam, sizes), d, n, args.steps, args.repeats),
                     "l1>0": ragged_case(bz, bz.GroupLasso.from_sizes(lam, sizes, 0.25 * lam), d, n, args.steps, args.repeats)}
        res[name]["l1_over_pure"] = res[name]["l1>0"]["avg_us_median"] / res[name]["l1=0"]["avg_us_median"]
    res["uniform8_over_norm_l21"] = res["uniform8"]["l1=0"]["avg_us_median"] / res["norm_l21_K8"]["avg_us_median"]
    return res


def run_solve(bz, f, g, dtype, steps, warmup, repeats):
    n = f.n
    prob = bz.Problem(f, g, bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
    prob.set_multipliers(np.full(n, 0.1, dtype), np.zeros(n, dtype))
    # (the first step size is given: with D = Free the estimate from grad L(x0 + 1) - grad L(x0) is 0 for the softmax)
    opts = bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(dtype).eps), gamma=1.0, adaptive=True).c_opts()
    prob.panoc_begin(opts, np.zeros(n, dtype))
    out = timed_steps(prob, steps, warmup, repeats)
    prob.profile_reset()
    prob.profile_enable(1 << 3)
    prob.panoc_steps(min(steps, 50))
    r = prob.profile2()["fb_step"]
    prob.profile_enable(False)
    out["fb_step"] = {"form_of_last_launch": r["form"], "avg_us": r["timed_ms"] * 1e3 / r["timed_launches"] if r["timed_launches"] else None,
                      "fraction_of_8TBs": r["timed_bytes"] / (r["timed_ms"] * 1e-3) / HBM_PEAK if r["timed_ms"] else None}
    st = prob.panoc_stats()
    out["n_backtracks"], out["n_gamma_halvings"] = int(st.n_backtracks), int(st.n_gamma_halvings)
    prob.close()
    return out


def worker(args):
    import bazinga_jl_amd as bz
    res = {}
    if args.worker == "ragged":
        res = ragged_worker(bz, args)
    elif args.worker.startswith("k"):
        K = int(args.worker[1:])
        n = args.n // K * K
        res = {"K": K, "n": n}
        for dtype in (np.float64, np.float32):
            d = bz.synth.l1_quadratic(args.n, dtype=dtype)
            r = {"group": fb_kernel(bz, bz.NormL21(d["lam"], K), d, n, dtype, args.steps),
                 "l1": fb_kernel(bz, bz.NormL1(d["lam"]), d, n, dtype, args.steps)}
            r["group_over_l1"] = r["group"]["avg_us"] / r["l1"]["avg_us"]
            res[np.dtype(dtype).name] = r
    else:
        dt = np.float64
        K = 8
        d = bz.synth.sparse_multinomial(args.m, args.nf, K, args.k, dt)
        f = bz.SparseMultinomial(d["indptr"], d["indices"], d["data"], d["labels"], args.nf, K)
        res = {"m": args.m, "n_f": args.nf, "K": K, "k": args.k, "n": f.n, "nnz": f.nnz, "dtype": "float64"}
        res["group"] = run_solve(bz, f, bz.NormL21(0.1, K), dt, args.steps, args.warmup, args.repeats)
        res["l1"] = run_solve(bz, f, bz.NormL1(0.1), dt, args.steps, args.warmup, args.repeats)
        res["group_over_l1_it_per_s"] = res["group"]["it_per_s_median"] / res["l1"]["it_per_s_median"]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="k<K>: the kernel comparison at group size K ; solve: the multinomial solves ; ragged: the group-pointer kind")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--groups", default=",".join(str(k) for k in GROUPS))
    ap.add_argument("--m", type=int, default=5_000_000)
    ap.add_argument("--nf", type=int, default=1_250_000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-solve", action="store_true", help="the kernel comparison alone")
    ap.add_argument("--ragged", action="store_true", help="the group Lasso over a group pointer instead (group_lasso_ragged.json)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--commit", default=None, help="the commit of the measured tree, recorded with the result")
    ap.add_argument("--limit", type=int, default=600, help="seconds per child process")
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return
    os.makedirs(args.out, exist_ok=True)

    def cmd(kind):
        opts = {"--n": args.n, "--m": args.m, "--nf": args.nf, "--k": args.k, "--steps": args.steps, "--warmup": args.warmup, "--repeats": args.repeats}
        return [sys.executable, os.path.abspath(__file__), "--worker", kind] + [str(v) for kv in opts.items() for v in kv]
    env = dict(os.environ)
    if args.ragged:
        res = {"commit": args.commit or commit_of_tree(), "ragged": run_child(cmd("ragged"), env, args.limit)}
        line = json.dumps(res)
        print(line)
        with open(os.path.join(args.out, "group_lasso_ragged.json"), "w") as fh:
            fh.write(line + "\n")
        return
    res = {"commit": args.commit or commit_of_tree(), "kernel": {}}
    for K in args.groups.split(","):
        res["kernel"]["K" + K] = run_child(cmd("k" + K), env, args.limit)
        sys.stderr.write(f"[bench_group_lasso] K = {K} done\n")
        sys.stderr.flush()
    if not args.no_solve:
        res["solve"] = run_child(cmd("solve"), env, args.limit)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, "group_lasso.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
