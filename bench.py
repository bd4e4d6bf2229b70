#!/usr/bin/env python3
"""bench.py — PANOCplus inner iterations/sec on the BASELINE headline workload.

    python bench.py --gpus N --steps K --warmup W [--full]

A plain run does what the headline figure needs and nothing else: set-up, the W warm-up and K timed iterations, the
outputs if --dump-outputs is given, the result line.  Every other measurement — the CPU baselines, the two-loop /
outer-iteration-3 / whole-solve side figures, the repeat blocks of a short K-step window, the RCCL line beside a
mailbox one — runs only with --full, which adds its keys to the same line; the keys of a plain line mean the same in both.

Workload (BASELINE.json configs[1], SURVEY.md §8(d) cfg 2): l1-regularised diagonal
quadratic, n = 10^7, fp64, f = sum x(0.5 q x - b), g = 2.5||x||_1 (soft-threshold prox),
c = Identity, D = Box[-1,1], LBFGS(5), mu = default_penalty_parameter!(x0 = 0) = 0.1,
y = 0 (outer iteration 1), tol = 0 so the solver never stops; synthetic splitmix64 data.

A "step" is one PANOCplus inner iteration (one Base.iterate(iter, state)).  Inputs and all
solver state are resident in HBM before the timed region starts.

N > 1 (one process per GPU, launched by torch.distributed.run): the SAME n = 10^7 problem
with x sharded in contiguous blocks over the ranks ("scaling": "strong"); the only data
exchanged are the reductions' partial scalars (RCCL all-gather of <= 10 doubles per rank).

Output: ONE JSON line on rank 0 (contract fields + "roofline" + "cpu_baseline", which is null without --full).

Roofline accounting (round 2): every fraction is BYTES THE IMPLEMENTED DATAFLOW MOVES / time / 8 TB/s, so it can
never exceed 1.  The library counts, per launch, the bytes the launch is designed to move (its read + write
streams x length x sizeof(T), bz_profile_get2); `roofline.achieved` divides the bytes of the dominant kernel's
timed launches by their HIP-event time, `roofline_iteration` divides the bytes of ALL launches of the timed
region by the wall time.  `roofline.traffic` is the PMC-measured HBM traffic per launch of that very
instantiation (profiles/pmc_traffic.json, matched on workload, size, template form and the hash of the kernel
sources; null if any of them differs).  How much fewer bytes that is than the reference's dataflow (SURVEY
§8(d): 65 passes per iteration on cfg 2) is reported apart, as `reference_dataflow_speedup`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
COPY_CEILING_GBS = 6290.0      # same guide: what a plain streaming copy reaches
M_LBFGS = 5
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_traffic.json")


def lib_sources_sha():
    """Hash of the sources the device library is built from: a PMC profile is attached to a bench line only if
    it was collected on this very code."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "bazinga.jl_amd", "csrc", "*.h")) +
                   glob.glob(os.path.join(ROOT, "bazinga.jl_amd", "csrc", "*.hip")) +
                   glob.glob(os.path.join(ROOT, "bazinga.jl_amd", "csrc", "*.inc")) +      # (the family instantiations)
                   [os.path.join(ROOT, "bazinga.jl_amd", "csrc", "Makefile"),               # (the compiler flags)
                    os.path.join(ROOT, "include", "bazinga_hip.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def pmc_lookup(workload, n, form):
    """(bytes per launch, source) of the PMC profile of kernel `form` on this workload and size, or (None, why)."""
    if not os.path.exists(PMC_FILE):
        return None, "no profiles/pmc_traffic.json"
    with open(PMC_FILE) as fh:
        pj = json.load(fh)
    sha = lib_sources_sha()
    stale = None
    for e in pj.get("entries", []):
        if e.get("workload") == workload and int(e.get("n", -1)) == int(n) and e.get("form") == form:
            if e.get("lib_sources_sha") != sha:
                stale = "profile of %s was collected on other kernel sources (%s, now %s)" % (form, e.get("lib_sources_sha"), sha)
                continue
            return int(e["hbm_bytes_per_launch"]), "profiles/pmc_traffic.json: %s [%s]" % (e.get("kernel"), e.get("collected"))
    return None, stale or "no PMC entry for (%s, n=%d, %s)" % (workload, n, form)


def runtime_env():
    return {k: os.environ.get(k) for k in ("HIP_FORCE_DEV_KERNARG", "HSA_ENABLE_INTERRUPT", "BZ_GFC", "BZ_XR", "BZ_UNI",
                                           "BZ_NT", "BZ_GRID", "BZ_PERSIST_BLOCKS") if os.environ.get(k) is not None}


def roofline_of(prof, cats, workload, n, steps):
    """The dominant kernel among `cats` (largest timed total) -> the roofline object; plus moved bytes per iteration
    over every launch of the timed region."""
    cand = {k: prof[k] for k in cats if prof[k]["timed_launches"]}
    dom = max(cand, key=lambda k: cand[k]["timed_ms"]) if cand else None
    moved_iter = sum(v["bytes"] for v in prof.values()) / max(1, steps)
    if dom is None:
        return None, moved_iter
    r = prof[dom]
    avg_s = r["timed_ms"] / 1e3 / r["timed_launches"]
    per_launch = r["timed_bytes"] / r["timed_launches"]
    achieved = per_launch / avg_s / 1e9
    traffic, src = pmc_lookup(workload, n, r["form"]) if r["form"] else (None, "the library reports no template form for this category")
    out = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": src,
           "kernel": "bz::" + (r["form"] or dom), "category": dom,
           "avg_launch_us": round(avg_s * 1e6, 3), "timed_launches": r["timed_launches"],
           "launches_per_iteration": round(r["launches"] / max(1, steps), 3),
           "moved_bytes_per_launch": int(per_launch),
           # (how many n-vectors one launch of this kernel streams: 9 = the m + 1 iterates, q, b in and x_d out; 10 / 11 with
           # mu*y / mu streamed, +1 whenever z is stored — comparable across windows of any K)
           "streams_per_launch": round(per_launch / (n * 8.0), 3) if workload.startswith(("cfg2", "cfg5")) else None,
           "frac_of_copy_ceiling": round(achieved / COPY_CEILING_GBS, 4),
           "traffic_rate": round(traffic / avg_s / 1e9, 1) if traffic else None,
           "traffic_frac": round(traffic / avg_s / 1e9 / HBM_PEAK_GBS, 4) if traffic else None,
           "wasted_traffic_ratio": round(traffic / per_launch, 4) if traffic else None}
    return out, moved_iter


def roofline_note(roof, ms_per_step):
    """The launches that carry a start / stop event pair are never pre-launched behind their gate and cost a few microseconds
    more than the plain ones they stand for: when the evented average of a once-per-iteration kernel exceeds the whole
    iteration's wall time, say so in the line (the direction is harmless: `frac` is understated)."""
    if roof and roof.get("launches_per_iteration", 0) >= 0.99 and roof["avg_launch_us"] > 1e3 * ms_per_step:
        roof["note"] = ("evented launches (avg %.1f us) are slower than the untimed ones they sample: the whole iteration takes "
                        "%.1f us; `achieved` / `frac` are understated by that margin" % (roof["avg_launch_us"], 1e3 * ms_per_step))
    return roof


def algorithmic_bytes_per_iter(n, w=8, m=M_LBFGS, n_al=2, n_fb=1, p_al=6):
    """B_iter = w n [(8m+1) + P_AL nAL + 4 nFB + 8]  (cfg 2: 65 passes)."""
    return w * n * ((8 * m + 1) + p_al * n_al + 4 * n_fb + 8)


DUMP_SAMPLE = 1 << 20          # --dump-outputs: at most this many elements per vector (8 MiB each in fp64)
DUMP_SEED = 20240607


def dump_sample_index(n):
    """The fixed, seeded sample of [0, n) that --dump-outputs writes of a long vector (all of it when it is short)."""
    if n <= DUMP_SAMPLE:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, size=DUMP_SAMPLE, dtype=np.int64))


def dump_outputs(out_dir, prob, n_global=None, lo=0, grp=None, rank=0):
    """--dump-outputs DIR: what a caller of the timed path receives after its last step — the solution z (what
    bz_panoc_finish returns), the iterate x, the fixed-point residual res and the solver's scalars — as DIR/<name>.npy.
    Vectors longer than DUMP_SAMPLE are written at the sample `dump_sample_index` picks (its global indices in
    index.npy).  Sharded runs: every rank reads its own block, rank 0 writes the concatenation in global order."""
    n_global = prob.n if n_global is None else n_global
    idx = dump_sample_index(n_global)
    mine = idx[(idx >= lo) & (idx < lo + prob.n)] - lo
    arrays = {}
    for name in ("z", "x", "res"):
        v = np.ascontiguousarray(prob.panoc_vector(name)[mine])
        if grp is not None:
            v = np.concatenate([np.frombuffer(b, dtype=v.dtype) for b in grp.allgather(v.tobytes())])
        arrays[name] = v
    if rank != 0:
        return
    arrays["index"] = idx.astype(np.float64)
    arrays["scalars"] = np.array([prob.panoc_scalars()[k] for k in prob.SCALAR_NAMES], dtype=np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    note(f"outputs of the last timed step written to {out_dir}: " + ", ".join(f"{k}{list(a.shape)}" for k, a in arrays.items()))


def note(msg):
    """progress line on stderr (a long silent run looks hung to the GPU box's watchdog)"""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def usable_cpus():
    """(threads to use, affinity count, cgroup quota in CPUs or None): the GPU box lists every host CPU in the
    affinity mask but its container is throttled to a CPU quota — more runnable threads than the quota only makes
    the OpenMP barriers spin against the throttle."""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            a, b = fh.read().split()
        if a != "max":
            quota = float(a) / float(b)
    except Exception:      # noqa: BLE001
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:      # noqa: BLE001
            pass
    use = aff if quota is None else max(1, min(aff, int(quota)))
    return use, aff, quota


def cpu_baseline(n, states):
    """The oracle's plain-C port (oracle/c/bz_oracle.c: one loop per Julia broadcast, no fusion) timed on
    this box's host cores on the same workload, bounded sample.  Two legs: single-threaded
    — what the reference's Julia broadcasts are — and the same loops split over the host threads."""
    from oracle import c_port
    import bazinga_jl_amd as bz
    d = bz.synth.l1_quadratic(n)
    mu, y, x0 = np.full(n, 0.1), np.zeros(n), np.zeros(n)
    kw = dict(lam=d["lam"], D="box", D_lo=d["lo"], D_hi=d["hi"], minimum_gamma=float(np.finfo(float).eps))
    c_port.load()
    note(f"cpu baseline, single-thread leg: {states} states at n={n}")
    t0 = time.perf_counter()
    c_port.panoc_run(d["q"], d["b"], mu, y, x0, states, **kw)
    dt = time.perf_counter() - t0
    out = {"value": round((states - 1) / dt, 4), "unit": "iterations/s", "cores": 1, "kind": "port",
           "sample": f"first {states - 1} PANOCplus iterations (plus the initial state) of the same n={n} "
                     f"workload, oracle/c/bz_oracle.c, single thread, {dt:.1f} s",
           "host_cpus": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)),
           # the real reference would be timed here if the box had Julia + ProximalAlgorithms
           "julia_on_box": __import__("shutil").which("julia") is not None}
    try:
        use, aff, quota = usable_cpus()
        threads = int(os.environ.get("BZ_BENCH_CPU_THREADS", "0")) or use
        out["cgroup_cpu_quota"] = quota
        os.environ["OMP_NUM_THREADS"] = str(threads)
        os.environ.setdefault("OMP_WAIT_POLICY", "passive")
        note(f"cpu baseline, all-cores leg: {threads} threads (affinity {aff}, cgroup quota {quota})")
        c_port.load(omp=True)
        st2 = 4 * states - 3
        c_port.panoc_run(d["q"], d["b"], mu, y, x0, 3, omp=True, **kw)          # thread pool + page warm-up
        t0 = time.perf_counter()
        c_port.panoc_run(d["q"], d["b"], mu, y, x0, st2, omp=True, **kw)
        dt2 = time.perf_counter() - t0
        out["all_cores"] = {"value": round((st2 - 1) / dt2, 4), "unit": "iterations/s", "cores": threads,
                            "sample": f"first {st2 - 1} iterations, same loops under `omp parallel for`, "
                                      f"{threads} threads = every CPU this container may use (affinity {aff}, "
                                      f"cgroup quota {quota}), {dt2:.1f} s"}
    except Exception as e:      # noqa: BLE001  (no OpenMP build on this box: the single-thread leg stands)
        out["all_cores"] = {"value": None, "note": repr(e)[:200]}
    return out


def cpu_baseline_oracle(workload, orc, n, ny, dtype, mu, y, x0, minimum_gamma, budget_s=14.0, max_states=40):
    """cfg 3 / cfg 4: the numpy restatement (oracle/bazinga_ref.py: one numpy statement per Julia broadcast) stepped
    on the same inputs for a bounded time.  Element-wise numpy is single-threaded, as Julia's broadcasts are; the
    dense products of cfg 4 go through the BLAS numpy links, with its default thread count (what `A * x` does in
    Julia) — `cores` says how many."""
    from oracle import bazinga_ref as ref
    blas_threads = 1
    if workload == "cfg4":
        try:
            from threadpoolctl import threadpool_info
            blas_threads = max([i.get("num_threads", 1) for i in threadpool_info() if i.get("user_api") == "blas"] or [1])
        except Exception:      # noqa: BLE001
            blas_threads = os.cpu_count() or 1
    if workload == "als":
        al = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), x0[:n])
        it = ref.PANOCplusIteration(al, ref.NonsmoothCostFunSlack(orc[1], orc[3], n, ny), x0, minimum_gamma=minimum_gamma)
    else:
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0)
        it = ref.PANOCplusIteration(al, ref.NonsmoothCostFun(orc[1]), x0, minimum_gamma=minimum_gamma)
    t0 = time.perf_counter()
    st = it.init()
    t_init = time.perf_counter() - t0
    k, t1 = 0, time.perf_counter()
    while k < max_states and (k < 3 or time.perf_counter() - t1 < budget_s):
        st = it.step(st)
        k += 1
    dt = time.perf_counter() - t1
    return {"value": round(k / dt, 4), "unit": "iterations/s", "cores": blas_threads, "kind": "port",
            "sample": f"first {k} PANOCplus iterations of the same {workload} workload (n={n}, ny={ny}, {np.dtype(dtype).name}) "
                      f"on oracle/bazinga_ref.py (numpy), {dt:.1f} s after a {t_init:.1f} s initial state",
            "host_cpus": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)),
            "julia_on_box": __import__("shutil").which("julia") is not None}


def whole_alps_rates(bz, oracles, n, ctx):
    """A whole Bazinga.alps solve of the workload (x0 = 0, y0 = 0, tol = 1e-6) through bz_alps_solve: inner
    iterations per second over the WHOLE call (alps.jl:27,103,115: elapsed_time brackets everything), (a) with the
    six n-vectors (x0, y0 in; x, y, s, mu out) in pageable host memory, as the Python / Julia hosts hand them over,
    and (b) with device pointers, which the C ABI accepts as well (hipMemcpyDefault): nothing but scalars crosses PCIe."""
    import ctypes as C
    L = bz._lib
    out = {}
    prob = bz.Problem(*oracles, n, n, np.float64, ctx)
    ao = L.AlpsOpts()
    L.load().bz_alps_default_opts(C.byref(ao), L.BZ_F64)
    po = bz.PANOCplus(tol=ao.inner_tol).c_opts()
    x0, y0 = np.zeros(n), np.zeros(n)
    for rep_i in range(2):      # (first call: page faults of fresh output arrays, lazy allocations)
        t0 = time.perf_counter()
        x, y, s, mu, st = prob.alps_solve(ao, po, x0, y0)
        dt = time.perf_counter() - t0
    out["host_pageable"] = {"ms": round(1e3 * dt, 3), "outer": int(st.tot_it), "inner": int(st.tot_inner_it),
                            "value": round(st.tot_inner_it / dt, 2), "unit": "inner iterations/s"}
    try:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        bufs = []
        for _ in range(6):
            p = C.c_void_p()
            if hip.hipMalloc(C.byref(p), n * 8) != 0:
                raise RuntimeError("hipMalloc failed")
            hip.hipMemset(p, 0, n * 8)
            bufs.append(p)
        hip.hipDeviceSynchronize()
        st2 = L.AlpsStats()
        for rep_i in range(2):
            t0 = time.perf_counter()
            L.check(L.load().bz_alps_solve(prob._h, C.byref(ao), C.byref(po), bufs[0], bufs[1], bufs[2], bufs[3], bufs[4],
                                           bufs[5], C.byref(st2)))
            dt2 = time.perf_counter() - t0
        # the same with bz_alps_opts.warm_start (an opt-in deviation from alps.jl:64): every subproblem
        # after the first starts at the step size the previous one ended with
        aw = L.AlpsOpts()
        C.memmove(C.byref(aw), C.byref(ao), C.sizeof(ao))
        aw.warm_start = 1
        st3 = L.AlpsStats()
        for rep_i in range(2):
            t0 = time.perf_counter()
            L.check(L.load().bz_alps_solve(prob._h, C.byref(aw), C.byref(po), bufs[0], bufs[1], bufs[2], bufs[3], bufs[4],
                                           bufs[5], C.byref(st3)))
            dt3 = time.perf_counter() - t0
        for p in bufs:
            hip.hipFree(p)
        out["device_pointers"] = {"ms": round(1e3 * dt2, 3), "outer": int(st2.tot_it), "inner": int(st2.tot_inner_it),
                                  "value": round(st2.tot_inner_it / dt2, 2), "unit": "inner iterations/s"}
        out["device_pointers_warm_start"] = {"ms": round(1e3 * dt3, 3), "outer": int(st3.tot_it), "inner": int(st3.tot_inner_it),
                                             "value": round(st3.tot_inner_it / dt3, 2), "unit": "inner iterations/s",
                                             "status": int(st3.status),
                                             "note": "opt-in: gamma carried across subproblems (not the reference's alps.jl:64)"}
        out["pcie_share_of_host_call"] = round(max(0.0, dt - dt2) / dt, 4)
    except Exception as e:      # noqa: BLE001
        out["device_pointers"] = {"value": None, "note": repr(e)[:200]}
    prob.close()
    return out


class SocketGroup:
    """Minimal process group over TCP (star through rank 0) for the launcher-side plumbing of N > 1:
    all-gather of small byte strings, barrier, max/min reductions.  torch.distributed would do, but
    importing torch makes libbazinga_hip bind to torch's bundled ROCm 7.0 HIP runtime instead of the
    system's 7.2 (measured: +20 us per iteration of launch overhead); the data path never uses this."""
    MAGIC = b"BZRV1"

    def __init__(self, rank, world, addr, port, timeout=120.0):
        import socket
        import struct
        self.rank, self.world, self._struct = rank, world, struct
        self.peers = []
        if rank == 0:
            srv = None
            for off in range(1, 40):
                try:
                    srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
                    srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
                    srv.bind((addr, port + off))
                    break
                except OSError:
                    srv.close()
                    srv = None
            if srv is None:
                raise RuntimeError("no free rendezvous port")
            srv.listen(world)
            srv.settimeout(timeout)
            slots = [None] * world
            while sum(c is not None for c in slots[1:]) < world - 1:
                c, _ = srv.accept()
                c.settimeout(timeout)
                hello = self._recvn(c, len(self.MAGIC) + 4)
                if hello[:len(self.MAGIC)] != self.MAGIC:
                    c.close()
                    continue
                r = struct.unpack("<i", hello[len(self.MAGIC):])[0]
                c.sendall(b"BZOK")
                slots[r] = c
            self.peers = slots
            srv.close()
        else:
            deadline = time.time() + timeout
            sock = None
            while sock is None and time.time() < deadline:
                for off in range(1, 40):
                    try:
                        c = socket.create_connection((addr, port + off), timeout=2.0)
                        c.settimeout(5.0)
                        c.sendall(self.MAGIC + struct.pack("<i", rank))
                        if self._recvn(c, 4) == b"BZOK":
                            c.settimeout(timeout)
                            sock = c
                            break
                        c.close()
                    except OSError:
                        continue
                if sock is None:
                    time.sleep(0.2)
            if sock is None:
                raise RuntimeError("could not reach rank 0")
            self.sock = sock

    @staticmethod
    def _recvn(c, n):
        buf = b""
        while len(buf) < n:
            chunk = c.recv(n - len(buf))
            if not chunk:
                raise RuntimeError("peer closed the rendezvous connection")
            buf += chunk
        return buf

    def _send(self, c, b):
        c.sendall(self._struct.pack("<i", len(b)) + b)

    def _recv(self, c):
        n = self._struct.unpack("<i", self._recvn(c, 4))[0]
        return self._recvn(c, n)

    def allgather(self, b: bytes):
        if self.rank == 0:
            parts = [b] + [self._recv(self.peers[r]) for r in range(1, self.world)]
            blob = b"".join(self._struct.pack("<i", len(x)) + x for x in parts)
            for r in range(1, self.world):
                self._send(self.peers[r], blob)
            return parts
        self._send(self.sock, b)
        blob = self._recv(self.sock)
        out, o = [], 0
        for _ in range(self.world):
            n = self._struct.unpack("<i", blob[o:o + 4])[0]
            out.append(blob[o + 4:o + 4 + n])
            o += 4 + n
        return out

    def barrier(self):
        self.allgather(b"")

    def reduce(self, x: float, op):
        vals = [self._struct.unpack("<d", v)[0] for v in self.allgather(self._struct.pack("<d", float(x)))]
        return op(vals)

    def close(self):
        for c in self.peers[1:] if self.rank == 0 else [self.sock]:
            try:
                c.close()
            except OSError:
                pass


class TorchGroup:
    """Same interface over torch.distributed (fallback if the TCP rendezvous cannot be set up)."""

    def __init__(self, rank, world, local_rank):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.rank, self.world = torch, dist, rank, world
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    def allgather(self, b: bytes):
        out = [None] * self.world
        self.dist.all_gather_object(out, b)
        return out

    def barrier(self):
        self.dist.barrier()
        self.torch.cuda.synchronize()

    def reduce(self, x, op):
        out = [None] * self.world
        self.dist.all_gather_object(out, float(x))
        return op(out)

    def close(self):
        self.dist.barrier()
        self.dist.destroy_process_group()


def run_block(prob, steps, begin):
    """`begin()` starts a fresh solve; W untimed iterations were done by the caller.  Times exactly `steps`
    iterations bracketed by device synchronisation."""
    prob.ctx.synchronize()
    t0 = time.perf_counter()
    prob.panoc_steps(steps)
    prob.ctx.synchronize()
    return time.perf_counter() - t0


def repeat_blocks(first_elapsed, steps, one_block):
    """When the timed K-step block is shorter than 100 ms, repeat it (fresh solve, same warm-up, each block timed
    the same way) and report the spread: `value` stays the first block's, as the contract says."""
    if first_elapsed >= 0.1:
        return None
    blocks = int(min(15, max(4, np.ceil(0.5 / max(first_elapsed, 1e-6)))))
    ts = [first_elapsed] + [one_block() for _ in range(blocks)]
    ms = sorted(1e3 * t / steps for t in ts)
    return {"blocks": len(ts), "ms_per_step_median": round(ms[len(ms) // 2], 5), "ms_per_step_min": round(ms[0], 5),
            "ms_per_step_max": round(ms[-1], 5), "value_median": round(1e3 / ms[len(ms) // 2], 3),
            "note": "the K-step block lasts < 100 ms: repeated from a fresh solve with the same warm-up; `value` is block 1"}


def event_period(steps, short_pass=False):
    """Sampling period of the in-library HIP events inside the timed region.  A launch that carries a start / stop event pair
    costs ~8 us more than a plain one (measured on cfg 3: 247.2 us per iteration with every 2nd launch timed, 238.2 with
    every 8th, 233.2 with every 32nd, 232.5 with none) and is never pre-launched behind its gate, so the timed region
    samples sparsely: about a dozen launches per kernel and K-step block (every 16th at the default K = 200: < 0.5 % of
    the block), never fewer than every 4th nor more than every 32nd.  BZ_BENCH_PERIOD overrides."""
    if os.environ.get("BZ_BENCH_PERIOD"):
        return int(os.environ["BZ_BENCH_PERIOD"])
    p = int(max(4, min(32, steps // 12)))
    if steps < 48:
        # a short block (the driver's K = 20): ONE evented launch per block — five of them were 2 % of the block's time; the
        # roofline average then also takes the samples of the repeat blocks (same workload, same K: `roofline.sampled_blocks`)
        p = int(max(4, steps))      # (the block's first launch: it follows the warm-up's last single step, so it is a plain launch anyway)
    # a short pass (an N = 8 shard: ~20 us) feels the ~14 us an evented, un-gated launch costs twice as much: half as often
    return min(32, 2 * p) if short_pass else p


def side_workload(args):
    """cfg 3 / cfg 4 (single GPU): the other BASELINE configs, same JSON shape; not the headline."""
    import bazinga_jl_amd as bz
    tuned = getattr(args, "runtime_tuning_mask", None)      # (main opted in already: a second call would report "nothing new set")
    if tuned is None:
        tuned = bz.runtime_tuning()
    eps64, eps32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
    slack = False
    if args.workload == "cfg3":
        d = bz.synth.obstacle_grid(2048)
        n = ny = 2048 * 2048
        dt, w = np.float64, 8
        oracles = lambda m: (m.Stencil5ptQuadratic(2048, 2048, d["b"]), m.Zero(), m.IdentityFunction(),
                             m.ClosedSet(m.IndBox(d["psi"], np.inf)))
        x0, mg = d["x0"], eps64
        ref_bytes = 63 * w * n            # 63 passes under the reference's dataflow
        label = "cfg3: 5-pt stencil QP on 2048^2 grid fp64, box D, g=Zero, LBFGS(5)"
    elif args.workload == "als":
        # the inner solve of Bazinga.als (src/algorithms/als.jl, src/utilities/auglagfunslack.jl) on the cfg 2
        # data — the same PANOCplus on the lifted vector xs = [x; s] with the block prox [prox_g; proj_D]
        n = ny = int(args.n or 10_000_000)
        d = bz.synth.l1_quadratic(n)
        dt, w = np.float64, 8
        slack = True
        oracles = lambda m: (m.DiagQuadratic(d["q"], d["b"]), m.NormL1(d["lam"]), m.IdentityFunction(),
                             m.ClosedSet(m.IndBox(-1.0, 1.0)))
        x0, mg = np.zeros(n + ny), eps64
        ref_bytes = 65 * w * (n + ny)     # (the cfg 2 model of SURVEY 8(d) applied to the lifted vector: the reference runs the same solver on it)
        label = "als: the slack form of cfg2 (l1-regularised diagonal quadratic, n=%d fp64, D=Box[-1,1]), inner vector [x; s], LBFGS(5)" % n
    else:
        ny, n = 8192, 65536
        d = bz.synth.basis_pursuit(ny, n, dtype=np.float32)
        dt, w = np.float32, 4
        oracles = lambda m: (m.Zero(), m.NormL1(1.0), m.DenseAffine(d["A"], d["b"]), m.ZeroSet())
        x0, mg = np.zeros(n, dt), eps32
        ref_bytes = 4 * ny * n * w        # A read twice per AL gradient, 2 AL gradients per iteration
        label = "cfg4: basis pursuit, dense A 8192x65536 fp32, l1 prox, D=ZeroSet, LBFGS(5)"
    prob = bz.Problem(*oracles(bz), n, ny, dt, slack=slack)
    mu, y = np.full(ny, 0.1, dt), np.zeros(ny, dt)
    prob.set_multipliers(mu, y)
    popts = bz.PANOCplus(tol=0.0, maxit=10 ** 12, minimum_gamma=mg,
                         directions=bz.LBFGS(M_LBFGS, compact=False if args.two_loop else None)).c_opts()

    def fresh():
        prob.panoc_begin(popts, x0)
        prob.panoc_steps(args.warmup)

    note(f"{args.workload}: warm-up {args.warmup} + {args.steps} timed iterations")
    fresh()
    prob.profile_reset()
    prob.profile_enable(True, period=event_period(args.steps))
    elapsed = run_block(prob, args.steps, None)
    prob.profile_enable(False)
    prof = prob.profile2()
    sc = prob.panoc_scalars()
    st = prob.panoc_stats()
    its = args.steps / elapsed
    cats = [k for k in prof if k not in ("collect", "all_gather")]
    roof, moved_iter = roofline_of(prof, cats, args.workload, n, args.steps)
    roofline_note(roof, 1e3 * elapsed / args.steps)
    if args.workload == "cfg4":
        # the two dense products stream the same matrix; the roofline object is the slower of the two, the other
        # one is listed beside it
        roof["other_gemv"] = {k: {"avg_launch_us": round(1e3 * prof[k]["timed_ms"] / prof[k]["timed_launches"], 3),
                                  "achieved": round(prof[k]["timed_bytes"] / prof[k]["timed_ms"] / 1e6, 1), "form": prof[k]["form"]}
                              for k in ("gemv", "k_gemv_t_mfma") if prof[k]["timed_launches"] and k != roof["category"]}
    rep = repeat_blocks(elapsed, args.steps, lambda: (fresh(), run_block(prob, args.steps, None))[1]) if args.full else None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, prob)
    cpu = None
    if args.full and not args.no_cpu_baseline:
        note(f"{args.workload}: cpu baseline on the numpy oracle")
        from oracle import bazinga_ref as ref
        cpu = cpu_baseline_oracle(args.workload, oracles(ref), n, ny, dt, mu, y, x0, mg)
    out = {
        "metric": "PANOC inner iterations/sec (%s)" % args.workload, "value": round(its, 3), "unit": "iterations/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 5),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64" if w == 8 else "f32",
        "data": "synthetic",
        "config": {"workload": label, "n": n, "ny": ny, "lbfgs_memory": M_LBFGS,
                   "lbfgs_form": "two-loop recursion" if args.two_loop else "library default for this oracle family",
                   "runtime_tuning": {"applied_mask": tuned, "env": runtime_env()}, "lib_sources_sha": lib_sources_sha()},
        "roofline": roof,
        "roofline_iteration": {"moved_bytes_per_iteration": int(moved_iter), "achieved": round(moved_iter * its / 1e9, 1),
                               "unit": "GB/s", "frac": round(moved_iter * its / 1e9 / HBM_PEAK_GBS, 4),
                               "note": "bytes every launch of the timed region is designed to move / wall time / 8 TB/s"},
        "reference_dataflow": {"bytes_per_iteration": int(ref_bytes), "speedup": round(ref_bytes / max(1.0, moved_iter), 3),
                               "note": "SURVEY §8(d) model of the reference's passes; NOT a roofline fraction"},
        "kernels": {k: {"launches_per_iteration": round(v["launches"] / args.steps, 2),
                        "avg_us": round(1e3 * v["timed_ms"] / v["timed_launches"], 2),
                        "moved_GBps": round(v["timed_bytes"] / v["timed_ms"] / 1e6, 1) if v["timed_bytes"] else None,
                        "form": v["form"] or None}
                    for k, v in prof.items() if v["timed_launches"]},
        "solver": {"gamma": sc["gamma"], "stop_norm": sc["stop_norm"], "k": int(sc["k"]), "lbfgs_mem": int(sc["lbfgs_mem"]),
                   "persist_fallbacks": int(st.persist_fallbacks)},
        "cpu_baseline": cpu}
    if rep:
        out["repeats"] = rep
    print(json.dumps(out), flush=True)
    prob.close()


def self_launch(n_ranks, argv, worker=None):
    """`python bench.py --gpus N` started plainly (no launcher: WORLD_SIZE unset): become the launcher.  N child processes,
    one per GPU, each with the environment torch.distributed.run would give it (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_ADDR / MASTER_PORT on 127.0.0.1); rank 0's stdout — the ONE JSON line — is relayed, everybody's stderr is
    inherited, and the exit code is the first non-zero one (the other ranks are then ended: the exact PIDs started here).
    Runs before this process has imported the library or made any GPU call.  `worker`: the script the ranks run (this
    file; tests pass a stub through BZ_BENCH_WORKER)."""
    import socket
    import subprocess
    worker = worker or os.environ.get("BZ_BENCH_WORKER") or os.path.abspath(__file__)
    with socket.socket() as sk:                       # a free port for the rendezvous (the group tries port + 1 ... + 39)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n_ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_ranks), LOCAL_WORLD_SIZE=str(n_ranks),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), BZ_BENCH_SELF_LAUNCHED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # (dmabuf IPC: the mailboxes and RCCL need it on this pool)
        procs.append(subprocess.Popen([sys.executable, worker] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    note(f"self-launch: {n_ranks} ranks, rendezvous 127.0.0.1:{port}")
    rc = 0
    out0 = b""
    try:
        import threading
        buf = []
        rd = threading.Thread(target=lambda: buf.append(procs[0].stdout.read()), daemon=True)
        rd.start()
        live = set(range(n_ranks))
        while live and rc == 0:
            for r in sorted(live):
                c = procs[r].poll()
                if c is not None:
                    live.discard(r)
                    if c != 0:
                        rc = c
                        note(f"self-launch: rank {r} exited with code {c}; ending the other ranks")
                        break
            time.sleep(0.05)
        if rc != 0:
            for r in sorted(live):
                procs[r].terminate()
            t_end = time.time() + 15.0
            for r in sorted(live):
                try:
                    procs[r].wait(max(0.1, t_end - time.time()))
                except subprocess.TimeoutExpired:
                    procs[r].kill()
        rd.join(30.0)
        out0 = buf[0] if buf else b""
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    sys.stdout.write(out0.decode("utf-8", "replace"))
    sys.stdout.flush()
    if rc == 0 and not any(ln.startswith("{") for ln in out0.decode("utf-8", "replace").splitlines()):
        note("self-launch: rank 0 printed no JSON line")
        rc = 3
    return rc


def fail(msg, rank=0, n_gpus=1):
    """Fail loudly: rank 0 prints a JSON line that says why (never a number for a configuration that was not measured),
    every rank exits non-zero."""
    if rank == 0:
        print(json.dumps({"metric": "PANOC inner iterations/sec", "value": None, "unit": "iterations/s", "n_gpus": n_gpus,
                          "error": str(msg)[:600]}), flush=True)
    raise SystemExit(f"[bench] rank {rank}: {msg}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n", "--size", dest="n", type=float, default=1e7,
                    help="global problem size (default: BASELINE cfg 2); spell it --size under torch.distributed.run, "
                         "whose own parser claims --n as an abbreviation")
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg3", "cfg4", "cfg5", "als"],
                    help="cfg2 (default, the headline metric); cfg3 2048^2 stencil QP; cfg4 dense-A basis "
                         "pursuit fp32; cfg5 = cfg2 at n=1e8")
    ap.add_argument("--family", default="diag-l1-box",
                    help="cfg2 / cfg5 with another element-wise oracle family f-g-D: f in diag|zero, g in "
                         "zero|l1|nonneg|l1box|indbox|indboxvec, D in box|boxvec|boxveclo|free|zero|vc|cc|eitheror|xor "
                         "(default: the BASELINE workload).  Same sizes, same JSON; every family has its own instantiation "
                         "of the one-pass kernel")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement (off by default: a plain run sets up, warms up, times --steps "
                         "iterations and prints its line): the CPU baselines, at N = 1 the two-loop, outer-iteration-3 and "
                         "whole-solve figures, the repeat blocks of a K-step window shorter than 100 ms, at N > 1 the RCCL "
                         "line beside a mailbox one")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--cpu-states", type=int, default=31)
    ap.add_argument("--no-fuse", action="store_true")
    ap.add_argument("--compact", action="store_true", help="(default) compact L-BFGS representation")
    ap.add_argument("--two-loop", action="store_true",
                    help="evaluate the L-BFGS operator by the two-loop recursion in the reference's operation order "
                         "(2M sequential reductions: 11 exchanges per iteration at N > 1)")
    ap.add_argument("--no-extras", action="store_true", help="with --full, N = 1: skip the two-loop, outer-iteration-3 and whole-solve side measurements")
    ap.add_argument("--no-p2p", action="store_true", help="N > 1: keep the RCCL all-gather for the scalar exchange")
    ap.add_argument("--no-rccl", action="store_true",
                    help="N > 1: do not create the RCCL communicator (p2p mailboxes only, checked for rank agreement "
                         "instead of against RCCL).  With BZ_BENCH_SAME_GPU=1 (all ranks on device 0) this rehearses "
                         "the N > 1 path on a one-GPU box, where RCCL refuses two ranks on one device")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step (z, x, res: a fixed "
                         "seeded sample of at most %d elements each, with its indices; the solver's scalars) as DIR/<name>.npy"
                         % DUMP_SAMPLE)
    args = ap.parse_args()

    # N > 1 without a launcher: start the N ranks ourselves, BEFORE anything touches the GPU (or loads the library)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and args.workload in ("cfg2", "cfg5"):
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))

    import bazinga_jl_amd as bz

    tuned = bz.runtime_tuning()      # explicit opt-in (the library no longer sets process-wide variables by itself)
    n = int(args.n)
    if args.workload == "cfg5":
        n = 100_000_000
    if args.workload in ("cfg3", "cfg4", "als"):
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            fail(f"--workload {args.workload} is a single-GPU line (the sharded forms of cfg 3 / cfg 4 are covered by "
                 "tests/test_gpu_p2p.py, not benchmarked)", int(os.environ.get("RANK", "0")), args.gpus)
        args.runtime_tuning_mask = tuned
        return side_workload(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        # (never time another rank count than the one asked for)
        fail(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks", rank, world)
    grp = None
    comm_id = None
    if world > 1:
        try:
            grp = SocketGroup(rank, world, os.environ.get("MASTER_ADDR", "127.0.0.1"),
                              int(os.environ.get("MASTER_PORT", "29500")))
        except Exception as e:      # noqa: BLE001
            print(f"[bench] TCP rendezvous failed ({e!r}); using torch.distributed", file=sys.stderr, flush=True)
            grp = TorchGroup(rank, world, local_rank)
        if not args.no_rccl:
            ids = grp.allgather(bz.Context.unique_id() if rank == 0 else b"")
            comm_id = ids[0]
    dev = local_rank if world > 1 else 0
    if os.environ.get("BZ_BENCH_SAME_GPU") == "1":
        dev = 0

    def agree(flag):
        return grp.reduce(flag, min) >= 1 if grp is not None else bool(flag)

    ctx, rccl_note = None, None
    try:
        if world == 1 or comm_id is not None:
            ctx = bz.Context(device=dev, rank=rank, nranks=world, comm_id=comm_id)
    except Exception as e:      # noqa: BLE001
        rccl_note = f"RCCL communicator failed: {e!r}"[:300]
        print(f"[bench] rank {rank}: {rccl_note}", file=sys.stderr, flush=True)
    if world > 1 and not agree(ctx is not None):
        if ctx is not None:
            ctx.close()
        ctx = None                              # no RCCL on this node: the p2p transport or nothing

    # the rank count RCCL itself reports (ncclCommCount): must be the launcher's world size
    rccl_nranks = ctx.comm_nranks() if ctx is not None and comm_id is not None else 0
    if world > 1 and ctx is not None and comm_id is not None and rccl_nranks != world:
        raise SystemExit(f"[bench] rank {rank}: RCCL communicator spans {rccl_nranks} ranks, launcher says {world}")

    lo_i, hi_i = bz.shard_bounds(n, rank, world)
    nl = hi_i - lo_i
    d = bz.synth.l1_quadratic(nl, start=lo_i)
    # The L-BFGS operator is evaluated in its compact representation: the whole iteration is ONE pass over
    # 2M + 11 vectors and one reduction phase (one cross-GPU exchange at N > 1), against 2M sequential
    # reductions for the two-loop recursion.  Same operator, alternate rounding — its iterates stay as close
    # to the fp64 oracle's as the two-loop kernels' do (oracle: LBFGSCompactOperator; tests:
    # test_compact_lbfgs_*; tests/stress/err_compact_vs_twoloop.py) — and it is what LBFGS(M) means by default on this
    # path (lbfgs_compact = 2, "auto").  --two-loop times the reference's order.
    compact = not args.two_loop
    popts = bz.PANOCplus(tol=0.0, maxit=10 ** 12, minimum_gamma=float(np.finfo(float).eps),
                         fuse=not args.no_fuse, directions=bz.LBFGS(M_LBFGS, compact=compact)).c_opts()

    fam = tuple(args.family.split("-"))
    if len(fam) != 3:
        raise SystemExit("--family must be f-g-D")
    headline = fam == ("diag", "l1", "box")

    def family_oracles():
        """(f, g, c, D) of --family on this rank's shard: the BASELINE data (q, b, lambda, [-1, 1]) wherever the family
        has the corresponding parameter, deterministic splitmix64 streams for the vector bounds"""
        fk, gk, dk = fam
        u6 = lambda k: bz.synth.uniform(k, nl, lo_i)
        f = bz.DiagQuadratic(d["q"], d["b"]) if fk == "diag" else bz.Zero()
        g = {"zero": lambda: bz.Zero(), "l1": lambda: bz.NormL1(d["lam"]), "nonneg": lambda: bz.NormL1Nonneg(d["lam"]),
             "l1box": lambda: bz.NormL1Box(d["lam"], u=0.25 + u6(6)), "indbox": lambda: bz.IndBox(-0.5, 0.5),
             "indboxvec": lambda: bz.IndBox(-(0.2 + 0.8 * u6(7)), 0.2 + 0.8 * u6(8))}[gk]()
        D = {"box": lambda: bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])),
             "boxvec": lambda: bz.ClosedSet(bz.IndBox(-(0.1 + 0.9 * u6(9)), 0.1 + 0.9 * u6(10))),
             "boxveclo": lambda: bz.ClosedSet(bz.IndBox(-(0.1 + 0.9 * u6(9)), np.inf)),
             "free": lambda: bz.FreeSet(), "zero": lambda: bz.ZeroSet(),
             "vc": lambda: bz.PairwiseSet("vc"), "cc": lambda: bz.PairwiseSet("cc"),
             "eitheror": lambda: bz.PairwiseSet("eitheror"), "xor": lambda: bz.PairwiseSet("xor")}[dk]()
        return f, g, bz.IdentityFunction(), D

    def make_problem(c, po=None, mu=None, y=None):
        p = bz.Problem(*family_oracles(), nl, nl, np.float64, c)
        p.set_multipliers(np.full(nl, 0.1) if mu is None else mu, np.zeros(nl) if y is None else y)
        p.panoc_begin(po or popts, np.zeros(nl))
        return p

    # N > 1: scalar exchange through peer-to-peer mailboxes (no collective call; the persistent two-loop
    # kernel runs sharded).  It is taken only if it reproduces the RCCL path's scalars on this node;
    # otherwise the RCCL all-gather path (always correct, slower) is timed.
    # Gated pre-launch is off by default in the library when there are several ranks: a launch that misses its gate
    # cannot be redone there.  It is asked for (BZ_GATE=1, read at every bz_panoc_begin) only after the p2p transport WITH
    # gated launches has reproduced, on this node, the plain launches of the RCCL path (or, without RCCL, the same bits on
    # every rank) — first with the gate, then without, each attempt on freshly connected mailboxes.
    transport = "none" if world == 1 else ("rccl" if ctx is not None else None)
    p2p_note = None
    ctx_rccl = None
    gate = "default" if world == 1 else "0"
    if world > 1:
        os.environ["BZ_GATE"] = "0"

    def p2p_context():
        """a context with everybody's mailbox mapped, or (None, why); the same group operations on every rank"""
        ok, c2, why = 1, None, None
        try:
            c2 = bz.Context(device=dev, rank=rank, nranks=world, comm_id=None)
            h = c2.p2p_export()
        except Exception as e:      # noqa: BLE001
            ok, why = 0, f"p2p export failed: {e!r}"[:300]
            h = b"\0" * 64
        hs = grp.allgather(h)
        dvs = [int(v) for v in grp.allgather(str(dev).encode())]
        if agree(ok):
            try:
                c2.p2p_connect(hs, dvs)
            except Exception as e:      # noqa: BLE001
                ok, why = 0, f"p2p connect failed: {e!r}"[:300]
        else:
            ok = 0
        if not agree(ok):
            if c2 is not None:
                c2.close()
            return None, why or "p2p setup failed on another rank"
        return c2, None

    if world > 1 and not (args.no_p2p and ctx is not None):
        keys = ("gamma", "f_x", "g_z", "stop_norm", "FBE")
        sa = None
        if ctx is not None:                     # the reference: the RCCL path, one step per call (plain launches)
            ok_a = 1
            try:
                pa = make_problem(ctx)
                for _ in range(24):
                    pa.panoc_step()
                sa = pa.panoc_scalars()
                pa.close()
            except Exception as e:      # noqa: BLE001
                ok_a, rccl_note = 0, f"RCCL reference run failed: {e!r}"[:300]
            if not agree(ok_a):
                sa = None
        same_gpu = os.environ.get("BZ_BENCH_SAME_GPU") == "1"
        notes = []
        for try_gate in (("0",) if same_gpu else ("1", "0")):
            ctx2, why = p2p_context()
            if ctx2 is None:
                notes.append(why)
                break                           # (no mailboxes: the gate makes no difference)
            os.environ["BZ_GATE"] = try_gate
            ok, sb, why, gated = 1, None, None, 0
            try:
                pb = make_problem(ctx2)
                pb.panoc_steps(24)              # (the library's own loop, as in the timed region: mailboxes (+ gated pre-launch))
                sb = pb.panoc_scalars()
                gated = int(pb.panoc_stats().n_gated_launches)
                pb.close()
                if sa is not None:
                    for key in keys:
                        if not abs(sa[key] - sb[key]) <= 1e-9 * max(1.0, abs(sa[key])):
                            ok, why = 0, f"p2p/rccl mismatch on {key}: {sb[key]} vs {sa[key]}"
                if not all(np.isfinite(sb[key]) for key in keys):
                    ok, why = 0, "p2p run produced non-finite scalars"
                if try_gate == "1" and gated == 0:
                    ok, why = 0, "no launch went through its gate"
            except Exception as e:      # noqa: BLE001  (a peer never answered: every rank times out alike)
                ok, why = 0, f"p2p run failed: {e!r}"[:300]
            # every rank must hold the same bits (they take the line-search decisions independently)
            mine = repr([sb[key] for key in keys]).encode() if sb is not None else b"none"
            if len(set(grp.allgather(mine))) != 1:
                ok, why = 0, why or "ranks disagree on the p2p scalars"
            if agree(ok):
                if ctx is not None:
                    ctx_rccl = ctx
                ctx, transport, gate = ctx2, "p2p", try_gate
                if sa is None:
                    notes.append("p2p checked for rank agreement only (no RCCL communicator: " + (rccl_note or "--no-rccl") + ")")
                break
            notes.append(("gated launches rejected: " if try_gate == "1" else "p2p rejected: ") + (why or "on another rank"))
            try:
                ctx2.close()
            except Exception:       # noqa: BLE001
                pass
        os.environ["BZ_GATE"] = gate if transport == "p2p" else "0"
        p2p_note = "; ".join(notes) or None
    if ctx is None:
        fail(f"no working scalar transport at N={world}: {rccl_note}; {p2p_note}", rank, world)
    def sync(ok=1):
        """Barrier + device drain that carries a health flag: the SAME group operation on every rank whatever
        happened locally, so one rank's failure cannot leave the others waiting in a different collective."""
        try:
            ctx.synchronize()
        except Exception:       # noqa: BLE001
            ok = 0
        if grp is not None:
            ok = 1 if grp.reduce(ok, min) >= 1 else 0
        try:
            ctx.synchronize()
        except Exception:       # noqa: BLE001
            ok = 0
        return ok

    ALG = ("k_twoloop_persist", "k_axpy_dot", "k_fused_sep", "k_dot", "k_fused_iterates")
    FUSED_FORMS = ("k_fused_sep", "k_fused_iterates")      # (category 1 also counts k_fused_compact's stored-pair forms)

    def timed_run(prob, steps, warmup, restart_opts=None):
        restart_opts = restart_opts or popts
        x0z = np.zeros(prob.n)
        x0z.fill(0.0)      # (pages touched now, not inside the timed bracket)
        """W untimed + K timed iterations on `prob`.  HIP events bound to each dispatch on the library's own
        stream (hipExtLaunchKernelGGL start/stop events): in the warm-up every kernel category is timed, to
        find the dominant kernel and fill the per-kernel table; in the timed region only every 8th launch of
        the dominant kernel carries events, so they do not perturb the pipeline."""
        ok, err, prof_warm, dom, st0 = 1, None, {}, "k_axpy_dot", None
        try:
            prob.profile_reset()
            prob.profile_enable(os.environ.get("BZ_BENCH_WARMPROF", "1") == "1")
            for i in range(warmup):
                prob.panoc_step()
                if i % 50 == 49 and i + 1 < warmup and prob.panoc_scalars()["stop_norm"] < 1e-12:
                    prob.panoc_begin(restart_opts, x0z)      # (as in the timed region, below)
            prof_warm = prob.profile()
            cands = {k: v for k, v in prof_warm.items() if k in ALG and v["launches"]}
            dom = max(cands, key=lambda k: cands[k]["total_ms"]) if cands else "k_axpy_dot"
            prob.profile_reset()
            mask = 1 << bz._lib.KERNEL_CATEGORIES.index(dom)
            if dom in FUSED_FORMS:      # both forms of the one-pass kernel: which one dominates is only known afterwards
                mask = sum(1 << bz._lib.KERNEL_CATEGORIES.index(k) for k in FUSED_FORMS)
            prob.profile_enable(mask, period=event_period(steps, prob.n < 3_000_000))
            st0 = prob.panoc_stats()
        except Exception as e:      # noqa: BLE001
            ok, err = 0, repr(e)[:300]
        ok = sync(ok)
        t0 = time.perf_counter()
        restarts, carry = 0, [0, 0, 0]
        if ok:
            try:
                # K iterations through the solver's own loop (bz_panoc_steps), 50 per library call.  With tol = 0
                # the solve never stops by itself; once it has converged to rounding (stop norm < 1e-12: about
                # iteration 280 of this workload, so never within the default K) it is started again from x0 INSIDE
                # the timed bracket — iterations at the noise floor, where every other pair has <s,y> <= 0 and is
                # skipped, are not what a solve does.  Every rank sees the same scalars, so all restart together.
                left = steps
                while left > 0:
                    c = min(left, 50)
                    prob.panoc_steps(c)
                    left -= c
                    if left > 0 and prob.panoc_scalars()["stop_norm"] < 1e-12:
                        stq = prob.panoc_stats()      # (bz_panoc_begin zeroes the counters: carry them over)
                        carry = [carry[0] + stq.n_fused_iters, carry[1] + stq.n_grad, carry[2] + stq.n_prox]
                        prob.panoc_begin(restart_opts, x0z)
                        restarts += 1
            except Exception as e:      # noqa: BLE001
                ok, err = 0, repr(e)[:300]
        ok = sync(ok)
        elapsed = time.perf_counter() - t0
        if grp is not None:
            elapsed = grp.reduce(elapsed, max)
        if not ok:
            return {"failed": err or "another rank failed"}
        prob.profile_enable(False)
        prof = prob.profile()
        if dom in FUSED_FORMS:
            dom = max(FUSED_FORMS, key=lambda k: prof[k]["total_ms"])
        return {"elapsed": elapsed, "st0": st0, "st1": prob.panoc_stats(), "sc": prob.panoc_scalars(),
                "prof": prof, "prof2": prob.profile2(), "prof_warm": prof_warm, "dom": dom, "restarts": restarts,
                "carry": carry}

    note(f"rank {rank}: timed run, {args.warmup} + {args.steps} iterations, n_local={nl}, transport={transport}")
    prob = make_problem(ctx)
    # A short window (the round driver's K = 20, W = 5 is 4 ms of GPU work) measured right after the problem was set up runs
    # 2-4 % below the blocks that follow it: the device comes out of idle while it is being timed.  An untimed solve of the same
    # workload first (half a second: a device that sat idle while the problem data was generated needs more than a few
    # milliseconds; BZ_BENCH_PRECOND=<seconds>, 0 turns it off), then the solve is started again and the W warm-up + K timed
    # steps run as the contract says.  Every rank takes the same path.
    precond = 0
    precond_s = float(os.environ.get("BZ_BENCH_PRECOND", "0.5"))      # (seconds of untimed iterations; 0: none)
    if precond_s > 0:
        try:
            # (every rank runs the same number of iterations: rank 0's clock decides, the count travels with the group)
            t_pre = time.perf_counter()
            while True:
                prob.panoc_steps(50)
                precond += 50
                if prob.panoc_scalars()["stop_norm"] < 1e-12:
                    prob.panoc_begin(popts, np.zeros(nl))
                more = 1 if (time.perf_counter() - t_pre < precond_s and precond < 20000) else 0
                if grp is not None:
                    more = int(grp.reduce(more, min))
                if not more:
                    break
        except Exception as e:      # noqa: BLE001  (the timed run reports what is wrong)
            note(f"rank {rank}: preconditioning solve failed: {e!r}")
        prob.panoc_begin(popts, np.zeros(nl))      # (as before every repeat block)
    R = timed_run(prob, args.steps, args.warmup)
    note(f"rank {rank}: timed run done" + (f": FAILED {R['failed']}" if "failed" in R else f": {args.steps / R['elapsed']:.1f} it/s"))
    if "failed" in R and transport == "p2p" and gate == "1":
        # every rank sees the same verdict (sync carries it): the same transport on fresh mailboxes, plain launches
        p2p_note = ((p2p_note + "; ") if p2p_note else "") + f"gated launches failed in the timed run ({R['failed']})"
        print(f"[bench] rank {rank}: {p2p_note}", file=sys.stderr, flush=True)
        gate = os.environ["BZ_GATE"] = "0"
        c3, why = p2p_context()
        if c3 is not None:
            ctx = c3
            prob = make_problem(ctx)
            R = timed_run(prob, args.steps, args.warmup)
        else:
            R = {"failed": f"{R['failed']}; then {why}"}
    if "failed" in R and transport == "p2p" and ctx_rccl is not None:
        p2p_note = ((p2p_note + "; ") if p2p_note else "") + f"p2p failed in the timed run ({R['failed']}); RCCL timed instead"
        print(f"[bench] rank {rank}: {p2p_note}", file=sys.stderr, flush=True)
        gate = os.environ["BZ_GATE"] = "0"
        ctx, transport = ctx_rccl, "rccl"
        ctx_rccl = None
        prob = make_problem(ctx)
        R = timed_run(prob, args.steps, args.warmup)
    if "failed" in R:
        fail(f"timed run failed: {R['failed']}", rank, world)
    # --full, K-step block shorter than 100 ms: repeat it from a fresh solve (same warm-up; every rank takes the same
    # decision from the max-over-ranks time) and report the spread beside the headline value
    repeats = None
    if args.full and R["elapsed"] < 0.1:
        nblk = int(min(15, max(4, np.ceil(0.5 / max(R["elapsed"], 1e-6)))))
        ts = [R["elapsed"]]
        R["prof2_blocks"] = [R["prof2"]]
        for _ in range(nblk):
            prob.panoc_begin(popts, np.zeros(nl))
            rb = timed_run(prob, args.steps, args.warmup)
            if "failed" in rb:
                break
            ts.append(rb["elapsed"])
            R["prof2_blocks"].append(rb["prof2"])
        msb = sorted(1e3 * t / args.steps for t in ts)
        repeats = {"blocks": len(ts), "ms_per_step_median": round(msb[len(msb) // 2], 5), "ms_per_step_min": round(msb[0], 5),
                   "ms_per_step_max": round(msb[-1], 5), "value_median": round(1e3 / msb[len(msb) // 2], 3),
                   "note": "the K-step block lasts < 100 ms: repeated from a fresh solve with the same warm-up; `value` is block 1"}
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, prob, n, lo_i, grp, rank)
    prob.close()
    # N > 1: north_star names RCCL for the scalar reductions — when the timed transport is the p2p mailboxes, the
    # RCCL all-gather transport is timed as well and printed beside it (with --full)
    rccl_extra = None
    if args.full and world > 1 and transport == "p2p" and ctx_rccl is not None:
        os.environ["BZ_GATE"] = "0"              # (gated launches were checked on the mailbox transport only)
        pr = make_problem(ctx_rccl)
        ctx_saved, ctx = ctx, ctx_rccl
        Rr = timed_run(pr, args.steps, args.warmup)
        ctx = ctx_saved
        pr.close()
        os.environ["BZ_GATE"] = gate
        rccl_extra = ({"value": round(args.steps / Rr["elapsed"], 3), "ms_per_step": round(1e3 * Rr["elapsed"] / args.steps, 5),
                       "gated_prelaunch": False}
                      if "failed" not in Rr else {"value": None, "note": Rr["failed"]})
    elapsed, st0, st1, sc, prof_all, prof_warm, dom = (R[k] for k in ("elapsed", "st0", "st1", "sc", "prof", "prof_warm", "dom"))

    # --full, N = 1 extras (rank 0 prints them beside the headline, they never replace it):
    #   two_loop : the same workload with the L-BFGS operator in the reference's two-loop operation order
    #   outer3   : the same workload inside outer iteration 3 (mu, y after two ALPS outer iterations: y != 0),
    #              SURVEY §8(d)
    extras = {}
    if args.full and world == 1 and not args.no_extras:
        note("extras: two-loop form and outer iteration 3")
        if compact:
            popts_tl = bz.PANOCplus(tol=0.0, maxit=10 ** 12, minimum_gamma=float(np.finfo(float).eps),
                                    fuse=not args.no_fuse, directions=bz.LBFGS(M_LBFGS, compact=False)).c_opts()
            p2 = make_problem(ctx, popts_tl)
            r2 = timed_run(p2, args.steps, args.warmup, popts_tl)
            p2.close()
            extras["two_loop"] = {"value": round(args.steps / r2["elapsed"], 3), "unit": "iterations/s",
                                  "ms_per_step": round(1e3 * r2["elapsed"] / args.steps, 5),
                                  "note": "directions=LBFGS(5) evaluated by the two-loop recursion in the reference's operation "
                                          "order (persistent register-resident kernel); same iterates up to rounding"}
        out3 = bz.alps(*family_oracles(), np.zeros(nl), np.zeros(nl), maxit=2, ctx=ctx)
        try:
            extras["whole_alps"] = whole_alps_rates(bz, family_oracles(), nl, ctx)
        except Exception as e:      # noqa: BLE001
            extras["whole_alps"] = {"note": repr(e)[:200]}
        p3 = make_problem(ctx, None, out3[9], out3[1])
        r3 = timed_run(p3, args.steps, args.warmup)
        p3.close()
        extras["outer3"] = {"value": round(args.steps / r3["elapsed"], 3), "unit": "iterations/s",
                            "ms_per_step": round(1e3 * r3["elapsed"] / args.steps, 5),
                            "note": "same workload with (mu, y) as left by two ALPS outer iterations (max|y| = %.3g)"
                                    % float(np.max(np.abs(out3[1])))}
    del d

    if rank == 0:
        its = args.steps / elapsed
        carry = R.get("carry", [0, 0, 0])
        n_fused = st1.n_fused_iters + carry[0] - st0.n_fused_iters
        n_al = (st1.n_grad + carry[1] - st0.n_grad) / args.steps
        n_fb = (st1.n_prox + carry[2] - st0.n_prox) / args.steps
        m = int(sc["lbfgs_mem"])
        # roofline: moved bytes of the dominant kernel's TIMED launches / their HIP-event time (<= 1 by construction);
        # the library counts per launch the bytes its streams must move (bz_profile_get2), whatever mix of template
        # forms ran (steady state of the default path: k_fused_compact<XR=2>: the m+1 last iterates, q, b (+ mu, mu*y
        # unless they travel as numbers) in, x_d out = 9..11 passes; 18..20 with stored pairs; the two-loop path:
        # k_twoloop_persist 4m passes + k_fused_sep 13)
        prof2 = R["prof2"]
        blocks = R.get("prof2_blocks") or [prof2]
        if len(blocks) > 1:
            # event samples of every K-step block (block 1's launch counts and bytes: `value` and the iteration figures stay block 1's)
            prof2 = {k: dict(v) for k, v in prof2.items()}
            for k in prof2:
                for key in ("timed_ms", "timed_launches", "timed_bytes"):
                    prof2[k][key] = sum(b[k][key] for b in blocks if k in b)
        roof, moved_iter = roofline_of(prof2, ALG, args.workload if headline else args.workload + ":" + args.family, nl, args.steps)
        if roof:
            roof["sampled_blocks"] = len(blocks)
        roofline_note(roof, 1e3 * elapsed / args.steps)
        # the reference's dataflow: 65 passes per iteration on this workload at m = 5 — a model of
        # what the reference moves, reported as a ratio, never as a roofline fraction
        ref_iter = algorithmic_bytes_per_iter(nl, m=max(1, m), n_al=2, n_fb=1)
        out = {
            "metric": ("PANOC inner iterations/sec, n=10^7 l1-quadratic" if n == 10_000_000 else "PANOC inner iterations/sec, n=%d l1-quadratic" % n)
            + ("" if headline else " (family %s)" % args.family),
            "value": round(its, 3), "unit": "iterations/s", "n_gpus": world, "transport_timed": transport, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 5),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": (args.workload + ": l1-regularised diagonal quadratic, n=%d fp64, soft-threshold prox_g, "
                                    "c=Identity, D=Box[-1,1], LBFGS(5), mu=0.1, y=0, tol=0" % n) if headline else
                       (args.workload + " with the oracle family f-g-D = %s, n=%d fp64, c=Identity, LBFGS(5), mu=0.1, y=0, tol=0"
                        % (args.family, n)),
                       "family": args.family,
                       "n": n, "n_per_gpu": nl, "lbfgs_memory": M_LBFGS,
                       "parallelism": "single GPU" if world == 1 else
                       f"x sharded over {world} GPUs, scalars exchanged by " +
                       ("peer-to-peer mailboxes over xGMI" if transport == "p2p" else "RCCL all-gather"),
                       "scalar_transport": transport, "p2p_note": p2p_note, "rccl_note": rccl_note,
                       "rccl_nranks": rccl_nranks,
                       "gated_prelaunch": {"default": "library default (on: one rank)", "1": "on (checked against plain launches on this node)",
                                           "0": "off"}[gate],
                       "gated_launches_in_timed_region": int(st1.n_gated_launches) - (int(st0.n_gated_launches) if not R.get("restarts") else 0),
                       "launcher": "self (bench.py --gpus N started its own ranks)" if os.environ.get("BZ_BENCH_SELF_LAUNCHED") else
                       ("torch.distributed.run / external" if world > 1 else "none"),
                       "lbfgs_form": "compact representation: one pass and one reduction phase per iteration" if compact
                       else "two-loop recursion (persistent kernel, 2M-1 grid phases)",
                       "runtime_tuning": {"applied_mask": tuned, "env": runtime_env()},
                       "untimed_iterations_before_warmup": precond,
                       "lib_sources_sha": lib_sources_sha()},
            "roofline": roof,
            "roofline_iteration": {"moved_bytes_per_iteration": int(moved_iter),
                                   "achieved": round(moved_iter * its / 1e9, 1), "unit": "GB/s",
                                   "frac": round(moved_iter * its / 1e9 / HBM_PEAK_GBS, 4),
                                   "note": "bytes every launch of the timed region is designed to move (this rank's shard) / "
                                           "wall time / 8 TB/s: includes the read-back launch and the host's turn-around"},
            "reference_dataflow": {"bytes_per_iteration": int(ref_iter),
                                   "speedup": round(ref_iter / max(1.0, moved_iter), 3),
                                   "rate_if_moved": round(ref_iter * its / 1e9, 1), "unit": "GB/s",
                                   "note": "SURVEY §8(d): 65 passes per iteration at m=5, nAL=2, nFB=1 under the reference's "
                                           "dataflow; the implemented dataflow moves `speedup` times fewer bytes.  NOT a "
                                           "roofline fraction."},
            "kernels_warmup": {k: {"launches_per_iteration": round(v["launches"] / max(1, args.warmup), 2),
                                   "avg_us": round(1e3 * v["total_ms"] / v["launches"], 2)}
                               for k, v in prof_warm.items() if v["launches"]},
            "solver": {"fused_iterations": int(n_fused), "al_grads_per_it": n_al, "prox_per_it": n_fb,
                       "restarts_in_timed_region": int(R.get("restarts", 0)),
                       "lbfgs_mem": m, "gamma": sc["gamma"], "stop_norm": sc["stop_norm"],
                       "k": int(sc["k"]), "persist_fallbacks": int(st1.persist_fallbacks)},
        }
        if repeats:
            out["repeats"] = repeats
        if rccl_extra:
            out["rccl_value"] = rccl_extra["value"]
            out["rccl"] = rccl_extra
        out.update(extras)
        if args.full and world == 1 and not args.no_cpu_baseline and headline:
            # bounded sample: ~10-30 s of CPU work whatever the size (the port runs ~2.5 it/s per 1e7 elements)
            states = max(4, int(round((args.cpu_states - 1) * min(1.0, 1.0e7 / n))) + 1)
            out["cpu_baseline"] = cpu_baseline(n, states)
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    ctx.close()
    if ctx_rccl is not None and ctx_rccl is not ctx:
        ctx_rccl.close()
    if grp is not None:
        grp.barrier()
        grp.close()


if __name__ == "__main__":
    main()
