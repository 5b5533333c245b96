"""The data-parallel step on the one GPU a test box has (the driver runs the real 2/4/8-GPU jobs):
(1) RCCL in a world of ONE rank, YOLO_DP_FORCE=1: process-group init with a device id, parameter broadcast, the
    bucketed async all-reduces on the side stream over views of the flat gradient buffer, the wait of the
    optimizer - every RCCL call of the N > 1 job, with a loss equal to the plain single-process step;
(2) two ranks sharing the GPU over gloo (RCCL refuses two ranks on one device): different data per rank, the
    1/world mean, replicas bit-identical after the steps.
bench.py is the program under test, launched the way the driver launches it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (warmup 2 + 3 timed steps: the step is captured after two eager steps, so the timed steps are hipGraph replays with the
# bucket all-reduces issued between the segments: tf2_yolo_amd/capture.py)
ARGS = ["--steps", "3", "--warmup", "2", "--batch", "4", "--no-cpu-baseline", "--no-kernel-timer"]


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def _env(**kw):
    env = dict(os.environ)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", **kw)
    return env


# (the eager form is what the tape records step by step; it is exercised by the first two steps of every tape / graph run)
@pytest.mark.parametrize("mode", ["tape", "graph"])
def test_rccl_single_rank_runs_every_collective_of_the_dp_step(mode):
    plain = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + ARGS, cwd=ROOT, env=_env(YOLO_STEP_MODE=mode),
                           capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-3000:]
    forced = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + ARGS, cwd=ROOT,
                            env=_env(YOLO_DP_FORCE="1", MASTER_PORT="29541", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                                     YOLO_STEP_MODE=mode),
                            capture_output=True, text=True, timeout=600)
    assert forced.returncode == 0, forced.stderr[-3000:]
    a, b = _json_line(plain.stdout), _json_line(forced.stdout)
    assert b["config"]["step_launch_mode"].startswith({"tape": "launch tape", "graph": "hipGraph", "eager": "eager"}[mode])
    assert b["config"]["replicas_in_sync"] is True and b["n_gpus"] == 1
    assert abs(a["config"]["loss"] - b["config"]["loss"]) <= 1e-3 * abs(a["config"]["loss"])


@pytest.mark.parametrize("mode", ["tape", "graph"])
def test_two_ranks_on_one_gpu_stay_in_sync_over_gloo(mode):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29543", "bench.py", "--gpus", "2"] + ARGS
    r = subprocess.run(cmd, cwd=ROOT, env=_env(YOLO_BENCH_SINGLE_DEVICE="1", YOLO_DIST_BACKEND="gloo", YOLO_STEP_MODE=mode),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 8 and j["scaling"] == "weak"
    assert j["config"]["replicas_in_sync"] is True
    if mode == "tape":
        # the bucket trace measures a REAL collective here (two ranks, gloo: device -> host -> loopback -> device): every
        # bucket's all-reduce finishes after it was ready, and moving tens of megabytes takes milliseconds, not the 0.01 ms
        # round 4's trace reported for every bucket (its `done` event was recorded behind the async call, not the collective)
        buckets = j["dp_trace"]["buckets"]
        assert len(buckets) >= 4
        assert all(d > r for _, r, d in buckets)
        assert all(d - r >= 1.0 for mb, r, d in buckets if mb >= 10.0), buckets


def test_bench_starts_its_own_ranks_without_a_torchrun_environment():
    """`python3 bench.py --gpus 2` as the driver's N = 1 line is called, no torchrun, no RANK / WORLD_SIZE: the parent (which
    makes no GPU call) starts two fresh rank processes, relays rank 0's JSON line and exits with the ranks' status. Here the two
    ranks share the one GPU of the test box over gloo (YOLO_BENCH_SINGLE_DEVICE=1); on an N-GPU node the same launcher puts one
    rank on each device over RCCL. A failing rank makes the launcher exit non-zero."""
    env = _env(YOLO_BENCH_SINGLE_DEVICE="1", YOLO_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + ARGS, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 8 and j["scaling"] == "weak"
    assert j["config"]["replicas_in_sync"] is True
    bad = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--batch", "-1"] + ARGS[:4], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0


def test_dp_step_timing_and_bucket_readiness_at_the_benchmark_batch():
    """The benchmark configuration (bs 32, launch tape) plain and with RCCL in a forced world of one rank -- side-stream
    all-reduces of every bucket, the waits on both gradient streams, the tape's host calls; one run of each, with a bound
    loose enough for the box's run-to-run drift
    (the measured cost is +1 % with 8 hardware queues; it was +13 % with the runtime's default of 4, which is what this test
    exists to catch: profiles/r04_b_dp_readiness.json). A world-1 all-reduce moves no data, so this says nothing about
    communication time; the functional coverage of the tape-mode DP step is test_rccl_single_rank_... above.
    The first gradient bucket must be ready within 5 ms of the start of backward (measured ~2 ms), and the buckets cover
    every trainable parameter of the model."""
    args = ["--steps", "8", "--warmup", "3", "--no-cpu-baseline", "--no-kernel-timer", "--no-extra-blocks"]
    last = {}
    for kind, env in (("plain", _env()),
                      ("forced", _env(YOLO_DP_FORCE="1", MASTER_PORT="29547", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + args, cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        last[kind] = _json_line(r.stdout)
    a, b = last["plain"], last["forced"]
    print("plain", a["ms_per_step"], "ms; forced RCCL world 1", b["ms_per_step"], "ms;", b["dp_trace"]["buckets"])
    assert b["config"]["step_launch_mode"].startswith("launch tape")
    assert b["config"]["replicas_in_sync"] is True and b["n_gpus"] == 1
    # the data-parallel tape step computes the SAME step as the plain one at the benchmark batch (same seeds, same 11 steps)
    assert abs(a["config"]["loss"] - b["config"]["loss"]) <= 1e-3 * abs(a["config"]["loss"]), (a["config"], b["config"])
    # ONE pair of runs on one box: 10 % covers the run-to-run drift (measured cost +1 %; the fault this guards against: +13 %)
    assert b["ms_per_step"] <= 1.10 * a["ms_per_step"], (a["ms_per_step"], b["ms_per_step"])
    buckets = b["dp_trace"]["buckets"]
    from tf2_yolo_amd import engine, graphs
    n_train, _ = engine.count_params(graphs.build_yolov3((416, 416, 3), 80))
    assert len(buckets) >= 4 and abs(sum(mb for mb, _, _ in buckets) - n_train * 4 / 1e6) < 1.0
    assert buckets[0][1] <= 5.0, buckets
    assert all(d >= r for _, r, d in buckets)


def test_allreduce_bucket_wrapper_with_a_one_rank_communicator():
    """yolo_allreduce_bucket (the thin RCCL wrapper of the C-ABI, for hosts that own their
    communicator): a one-rank RCCL communicator created here through the RCCL torch bundles (ncclGetUniqueId /
    ncclCommInitRank), two slices of a flat buffer reduced in place on a side stream -- a sum over one rank leaves the values
    as they are, and the call must have run on the given stream (the wrapper resolves ncclAllReduce in the process at its
    first call: the same RCCL copy, never a second one)."""
    import ctypes
    import glob
    import torch
    from tf2_yolo_amd import _lib
    from tf2_yolo_amd._lib import check
    paths = glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so*"))
    assert paths, "torch ships no librccl.so here"
    rccl = ctypes.CDLL(paths[0], mode=ctypes.RTLD_GLOBAL)

    class UniqueId(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_char * 128)]
    uid = UniqueId()
    rccl.ncclGetUniqueId.argtypes = [ctypes.POINTER(UniqueId)]
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
    torch.cuda.set_device(0)
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    try:
        flat = torch.randn(3_000_000, device="cuda")
        want = flat.clone()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        lib = _lib.load()
        for lo, hi in ((0, 1_000_000), (1_000_000, 3_000_000)):
            view = flat[lo:hi]
            check(lib.yolo_allreduce_bucket(comm, ctypes.c_void_p(view.data_ptr()), hi - lo, ctypes.c_void_p(st.cuda_stream)),
                  "yolo_allreduce_bucket")
        st.synchronize()
        assert torch.equal(flat, want)
        assert lib.yolo_allreduce_bucket(None, ctypes.c_void_p(flat.data_ptr()), 16, ctypes.c_void_p(st.cuda_stream)) != 0
    finally:
        rccl.ncclCommDestroy(comm)
