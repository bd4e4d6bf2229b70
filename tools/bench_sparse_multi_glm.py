#!/usr/bin/env python
"""Measure the sparse multi-response GLM f (BZ_F_SPARSE_MULTI_GLM) on the MI355X.  bench.py is not involved.

    python tools/bench_sparse_multi_glm.py      # synth.sparse_multiresponse(m = 5e6, n_f = 1.25e6, K, 5) at K = 2, 8, 32 with the
                                                # least-squares and the logistic loss (n = n_f K: 10^7 at K = 8), g = NormL1,
                                                # c = Identity, D = Free, fp64, beside SparseMultinomial at the same K and the
                                                # scalar SparseLeastSquares (n = n_f) on the SAME matrix, in the same session

Prints ONE JSON line and writes it to <out>/sparse_multi_glm.json: per run the iterations per second (warm-up steps, then
`repeats` timed calls of bz_panoc_steps: median, minimum and maximum), and, from further runs of the same workers under
`rocprofv3 --kernel-trace --stats` (skipped with a note where that tool is missing), each row kernel's time per launch — the
median over the launches of the trace with its minimum and maximum — with its share of the HBM peak by the byte model, and the
first launch k_spmm_glm_r beside k_spmm_softmax_r at the same K and beside k_spmv_ls_r.  One child process per K runs the
softmax and the two losses one after the other (the rows of the trace are told apart by the kernel's MODE argument); every GPU
step is a child under a time limit of its own, and the first one that fails ends the run.

(The multi-response runs take the default PANOCplus: every loss here sees the step-size probe x0 + 1.  The softmax run is
given gamma = 1 with adaptive = True, as tools/bench_sparse_multinomial.py gives it.)"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_sparse import HBM_PEAK, run_problem                         # noqa: E402
from tools.bench_sparse import child as run_child                            # noqa: E402
from tools.bench_sparse_logistic import commit_of_tree                       # noqa: E402
from tools.bench_sparse_ls import ls_bytes                                   # noqa: E402
from tools.bench_sparse_multinomial import mn_bytes, plan_k, run_multinomial  # noqa: E402

CLASSES = (2, 8, 32)
LOSSES = {"ls": "least_squares", "logit": "logistic"}
MODES = {"101": "ls", "102": "logit"}      # SPMM_GLM_MODE0 + BZ_LOSS_*: the kernel's last template argument


def mg_bytes(f, dtype):
    """the byte model of the three K-wide passes: mn_bytes' with K values of B per row (and K of R) in the pass over A_f"""
    sz, K = np.dtype(dtype).itemsize, f.n_classes
    out = mn_bytes(f, dtype)
    L, nv, seg = plan_k(f.indptr, f.nnz, K)
    out["k_spmm_glm_r"] = {"L": L, "segmented": seg, "bytes": f.nnz * (sz + 4) + (nv + 1) * 8 + (nv * 8 if seg else 0) +
                           (f.n + (2 * K + (f.weights is not None)) * f.m) * sz}
    del out["k_spmm_softmax_r"]
    return out


def kernel_times(directory):
    """per row kernel of the trace — keyed by its name, and for k_spmm_glm_r by its loss — the launches and the median, minimum
    and maximum duration of one launch (us)"""
    durations = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Kernel_Name", "").replace("void bz::", "").replace(" ", "")
            m = re.match(r"(k_sp(?:mv|mm)_\w+)<([^>]*)>", name)
            if not m:
                continue
            key = m.group(1)
            if key == "k_spmm_glm_r":
                key += ":" + MODES.get(m.group(2).split(",")[-1], m.group(2).split(",")[-1])
            durations.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not durations:
        raise SystemExit(f"no row kernel in the kernel trace under {directory}: nothing more is started")
    return {k: {"calls": len(v), "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in durations.items()}


def first_kernel(kind):
    """the trace's key of the launch over A_f of a kind (ls, mn<K>, ls<K>, logit<K>)"""
    if kind == "ls":
        return "k_spmv_ls_r"
    name = re.match(r"[a-z]+", kind).group(0)
    return "k_spmm_softmax_r" if name == "mn" else "k_spmm_glm_r:" + name


def worker(args):
    import bazinga_jl_amd as bz
    dt = np.float64
    res = {"dtype": "float64", "m": args.m, "n_f": args.nf, "k": args.k, "runs": {}}
    rest = (bz.NormL1(0.1), bz.IdentityFunction(), bz.FreeSet())
    for kind in args.worker.split(","):
        name, K = re.match(r"([a-z]+)(\d*)", kind).groups()
        if kind == "ls":                                      # the yardstick: the scalar kind on the same matrix
            d = bz.synth.sparse_lasso(args.m, args.nf, args.k, dt)
            f = bz.SparseLeastSquares(d["indptr"], d["indices"], d["data"], d["b"], args.nf)
            r = {"n": f.n, "model": ls_bytes(f, dt), "run": run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)}
        elif name == "mn":                                    # the softmax at the same K
            d = bz.synth.sparse_multinomial(args.m, args.nf, int(K), args.k, dt)
            f = bz.SparseMultinomial(d["indptr"], d["indices"], d["data"], d["labels"], args.nf, int(K))
            r = {"n": f.n, "K": int(K), "model": mn_bytes(f, dt), "run": run_multinomial(bz, f, dt, args.steps, args.warmup, args.repeats)}
        else:
            d = bz.synth.sparse_multiresponse(args.m, args.nf, int(K), args.k, dt, LOSSES[name])
            f = bz.SparseMultiGLM(d["indptr"], d["indices"], d["data"], d["B"], args.nf, LOSSES[name])
            r = {"n": f.n, "K": int(K), "loss": LOSSES[name], "model": mg_bytes(f, dt),
                 "run": run_problem(bz, (f,) + rest, f.n, f.n, dt, args.steps, args.warmup, args.repeats)}
        res["nnz"] = f.nnz
        res["runs"][kind] = r
        sys.stderr.write(f"[bench_sparse_multi_glm] {kind} done\n")
        sys.stderr.flush()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="comma-separated kinds of ls, mn<K>, ls<K>, logit<K>")
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
    groups = [["ls"]] + [[p + c for p in ("mn", "ls", "logit")] for c in args.classes.split(",")]      # a process per K

    def cmd(kinds, **over):
        opts = {"--m": args.m, "--nf": args.nf, "--k": args.k, "--steps": args.steps, "--warmup": args.warmup, "--repeats": args.repeats}
        opts.update(over)
        return [sys.executable, os.path.abspath(__file__), "--worker", ",".join(kinds)] + [str(v) for kv in opts.items() for v in kv]

    def child(command, environment, what):
        out = run_child(command, environment, args.limit)
        sys.stderr.write(f"[bench_sparse_multi_glm] {what} done\n")
        sys.stderr.flush()
        return out
    env = dict(os.environ)
    env.pop("BZ_SPLS_FUSED", None)
    env.pop("BZ_SPMV_L", None)
    res = {"commit": args.commit or commit_of_tree(), "runs": {}}
    for kinds in groups:
        r = child(cmd(kinds), env, "it/s of " + ",".join(kinds))
        res.update({k: v for k, v in r.items() if k != "runs"})
        res["runs"].update(r["runs"])
    res["it_per_s_median"] = {k: v["run"]["it_per_s_median"] for k, v in res["runs"].items()}
    rocprof = shutil.which("rocprofv3")
    if rocprof:
        res["per_kernel"] = {}
        for kinds in groups:
            d = os.path.join(args.out, "rocprof_sparse_multi_glm_" + kinds[0])
            shutil.rmtree(d, ignore_errors=True)
            child([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd(kinds, **{"--steps": 40, "--repeats": 1}),
                  env, "rocprofv3 " + ",".join(kinds))
            kt = kernel_times(d)
            shutil.rmtree(d, ignore_errors=True)
            for kind in kinds:                                # the first launch of every kind, with its share of the HBM peak
                key = first_kernel(kind)
                v = kt.get(key)
                if v:
                    b = res["runs"][kind]["model"].get(key.split(":")[0])
                    res["per_kernel"][kind] = dict(v, kernel=key.split(":")[0],
                                                   fraction_of_8TBs=b["bytes"] / (v["median_us"] * 1e-6) / HBM_PEAK if b else None)
            # (the launches over A_f' of the process's kinds share their names: together)
            res["per_kernel"]["rows_of_At:" + "+".join(kinds)] = {k: v for k, v in kt.items() if k.startswith(("k_spmm_t", "k_spmv_ls_t"))}
        base = res["per_kernel"].get("ls")
        res["glm_r_against"] = {}
        for c in args.classes.split(","):
            sm = res["per_kernel"].get("mn" + c)
            for p in ("ls", "logit"):
                v = res["per_kernel"].get(p + c)
                if v and sm and base:
                    res["glm_r_against"][p + c] = {
                        "K": int(c), "glm_r_us": v["median_us"], "softmax_r_us": sm["median_us"], "ls_r_us": base["median_us"],
                        "against_softmax_r": v["median_us"] / sm["median_us"], "against_softmax_r_min": v["min_us"] / sm["max_us"],
                        "against_softmax_r_max": v["max_us"] / sm["min_us"], "scalar_launches": v["median_us"] / base["median_us"],
                        "scalar_launches_per_response": v["median_us"] / base["median_us"] / int(c)}
    else:
        res["per_kernel"] = "rocprofv3 not found: iterations per second only"
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.out, "sparse_multi_glm.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
