"""`python bench.py --gpus N` started plainly (no torch.distributed.run around it) must start its own N ranks before any
GPU call, relay rank 0's one JSON line and propagate a failure (VERDICT r02 "Next" item 3).  World size 2 on the CPU with a
stub worker in place of the measuring code (BZ_BENCH_WORKER): what is under test is the launcher — environment of the ranks,
rendezvous, relay, exit code, clean-up of the surviving ranks."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r'''
import json, os, sys, time
sys.path.insert(0, %(root)r)
import bench
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert os.environ["LOCAL_RANK"] == os.environ["RANK"] and os.environ["MASTER_ADDR"] == "127.0.0.1"
g = bench.SocketGroup(rank, world, os.environ["MASTER_ADDR"], int(os.environ["MASTER_PORT"]), timeout=60)
parts = g.allgather(str(rank).encode())
if %(mode)r == "fail" and rank == 1:
    sys.exit(7)
if %(mode)r == "fail":
    time.sleep(600)          # rank 0 would wait for its peer for ever: the launcher must end it
g.barrier()
if rank == 0:
    print("not the json line")
    print(json.dumps({"metric": "stub", "value": len(parts), "n_gpus": world, "argv": sys.argv[1:],
                      "self": os.environ.get("BZ_BENCH_SELF_LAUNCHED")}), flush=True)
g.close()
'''


def _launch(tmp_path, mode, *args, env_extra=None):
    stub = tmp_path / f"stub_{mode}.py"
    stub.write_text(STUB % {"root": ROOT, "mode": mode})
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["BZ_BENCH_WORKER"] = str(stub)
    env.update(env_extra or {})
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=180)
    return r, time.time() - t0


def test_self_launch_starts_the_ranks_and_relays_rank0(tmp_path):
    r, _ = _launch(tmp_path, "ok", "--gpus", "2", "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["value"] == 2 and d["n_gpus"] == 2 and d["self"] == "1"
    assert d["argv"] == ["--gpus", "2", "--steps", "3", "--warmup", "1"]      # the ranks get the caller's arguments unchanged


def test_self_launch_propagates_a_failing_rank_and_ends_the_others(tmp_path):
    r, dt = _launch(tmp_path, "fail", "--gpus", "2")
    assert r.returncode == 7, (r.returncode, r.stderr[-2000:])
    assert dt < 60, dt                                                        # rank 0 (asleep for 600 s) was ended
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_rank_count_mismatch_fails_loudly_with_a_reason():
    """under a launcher that started another number of ranks than --gpus says: a JSON line with the reason, rc != 0 — never a
    number for a configuration that was not the one asked for"""
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode != 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["value"] is None and "WORLD_SIZE=3" in d["error"]


def test_single_gpu_invocation_does_not_self_launch():
    """--gpus 1 (the default) is this very process: nothing is spawned (no GPU here: the import of the library is as far as it
    gets before a context is needed — the point is that self_launch is not on that path)"""
    sys.path.insert(0, ROOT)
    import bench
    import inspect
    src = inspect.getsource(bench.main)
    assert "args.gpus > 1 and \"WORLD_SIZE\" not in os.environ" in src
    assert src.index("self_launch(") < src.index("import bazinga_jl_amd")      # before the library is even loaded


def test_full_is_an_option_and_off_by_default():
    """the side measurements hang on --full: the parser knows the option (what it switches is checked on the GPU, in
    test_gpu_bench_contract.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0 and "--full" in r.stdout
