#!/usr/bin/env python
"""Measure the ALS inner iteration with a dense affine constraint on the MI355X.  bench.py is not involved.

    python tools/bench_als_dense.py                        # cfg 4's shape: A 8192 x 65536 fp32, basis pursuit
    python tools/bench_als_dense.py --shape 2048 16384     # a smaller matrix of the same generator

Prints ONE JSON line and writes it to <out>/als_dense.json:

  als               the slack form (bz.Problem(..., slack=True)) on xs = [x; s]: inner iterations per second (warm-up steps,
                    then `repeats` timed calls of bz_panoc_steps(K), which return when their results are on the host:
                    median, minimum, maximum), and from HIP events on every dispatch of a further run the time of each
                    kernel category per iteration and, for the two passes over A (k_gemv_n in category `gemv`,
                    k_gemv_t_mfma in its own), bytes moved / time / 8 TB/s;
  alps_two_kernel   the yardstick, measured in the same process on the same matrix: the alps inner iteration with the
                    one-pass kernel (BZ_DENSE_FUSED=0, read when the problem is created) and the affine images
                    (affine_refresh = 0) switched off — the two-kernel form of the AL gradient, which is the form the slack
                    iteration takes;
  als_over_alps     the ratio of the two median rates.

The measuring process is a child under a time limit of its own; if it fails nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # bytes / s


def timed_steps(prob, K, warmup, repeats):
    prob.panoc_steps(warmup)
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        prob.panoc_steps(K)
        rates.append(K / (time.perf_counter() - t0))
    return {"K": K, "warmup": warmup, "repeats": repeats, "it_per_s_median": statistics.median(rates),
            "it_per_s_min": min(rates), "it_per_s_max": max(rates)}


def per_kernel(prob, steps):
    """every dispatch of `steps` iterations carries HIP events: per category the launches and the time per iteration;
    for the passes over A the rate of the bytes they were designed to move"""
    prob.profile_reset()
    prob.profile_enable(True)
    st0 = prob.panoc_stats()
    prob.panoc_steps(steps)
    st1 = prob.panoc_stats()
    pr = prob.profile2()
    prob.profile_enable(False)
    out = {"steps": steps, "n_grad": st1.n_grad - st0.n_grad, "n_backtracks": st1.n_backtracks - st0.n_backtracks,
           "n_gamma_halvings": st1.n_gamma_halvings - st0.n_gamma_halvings, "categories": {}}
    total = 0.0
    for name, r in pr.items():
        if not r["launches"]:
            continue
        e = {"launches_per_iteration": r["launches"] / steps, "us_per_iteration": r["timed_ms"] * 1e3 / steps,
             "us_per_launch": r["timed_ms"] * 1e3 / max(1, r["timed_launches"]), "form_of_last_launch": r["form"],
             "bytes_per_iteration": r["bytes"] / steps}
        if name in ("gemv", "k_gemv_t_mfma") and r["timed_ms"]:
            e["fraction_of_8TBs"] = r["timed_bytes"] / (r["timed_ms"] * 1e-3) / HBM_PEAK
        total += e["us_per_iteration"]
        out["categories"][name] = e
    out["kernel_us_per_iteration"] = total
    return out


def measure(bz, dev, n, ny, dtype, slack, args, **sub_kw):
    prob = bz.Problem(*dev, n, ny, dtype, slack=slack)
    prob.set_multipliers(np.full(ny, 0.1, dtype), np.zeros(ny, dtype))
    sub = bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(dtype).eps), **sub_kw)
    prob.panoc_begin(sub.c_opts(), np.zeros(prob.n, dtype))
    out = timed_steps(prob, args.steps, args.warmup, args.repeats)
    out["one_iteration"] = per_kernel(prob, args.profile_steps)
    st = prob.panoc_stats()
    out["n_fused_iters"], out["n_affine_images"], out["n_dense_onepass"] = st.n_fused_iters, st.n_affine_images, st.n_dense_onepass
    prob.close()
    return out


def worker(args):
    import bazinga_jl_amd as bz
    ny, n = args.shape
    dtype = np.float32
    d = bz.synth.basis_pursuit(ny, n, dtype=dtype, density=0.01)
    dev = (bz.Zero(), bz.NormL1(1.0), bz.DenseAffine(d["A"], d["b"]), bz.ZeroSet())
    res = {"shape": [ny, n], "dtype": "float32", "matrix_bytes": ny * n * 4}
    res["als"] = measure(bz, dev, n, ny, dtype, True, args)
    os.environ["BZ_DENSE_FUSED"] = "0"          # (read when the problem is created: the two-kernel form of the AL gradient)
    res["alps_two_kernel"] = measure(bz, dev, n, ny, dtype, False, args, affine_refresh=0)
    res["als_over_alps"] = res["als"]["it_per_s_median"] / res["alps_two_kernel"]["it_per_s_median"]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--shape", type=int, nargs=2, default=[8192, 65536], help="rows and columns of A (columns: a multiple of 64)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=540, help="seconds for the measuring process")
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return
    os.makedirs(args.out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--shape", *map(str, args.shape), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--profile-steps", str(args.profile_steps)]
    env = dict(os.environ)
    env.pop("BZ_DENSE_FUSED", None)
    res = child(cmd, env, args.limit)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, "als_dense.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
