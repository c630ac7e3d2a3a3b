"""N>1 path on CPU: world_size-2 gloo processes shard the frame's blocks, render, and reduce the film."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_gloo_block_shards_reduce_to_the_whole_frame(tmp_path, world, oracle):
    out = tmp_path / "result.txt"
    port = free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_dist_worker.py"), str(out)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=540)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    w, r, err, total, whole_samples, slowest, w0 = out.read_text().split()
    assert int(w) == world and int(r) == 0
    assert float(err) < 1e-6                       # sum of the shards == the unsharded render
    assert int(total) == int(whole_samples) == 96 * 64 * 4
    assert float(slowest) == world                 # max over ranks
    assert float(w0) > 0                           # rank 0 rendered some blocks itself


def test_single_process_helpers_are_noops():
    import torch
    from mitsuba_amd import distributed as D
    t = torch.ones(2, 2, 5)
    assert D.reduce_film(t) is t and D.max_over_ranks(3.0) == 3.0 and D.sum_over_ranks(4) == 4.0
    D.barrier()
    assert D.Solo.reduce_film(t) is t and D.Solo.max_over_ranks(2.5) == 2.5 and D.Solo.sum_over_ranks(7) == 7.0
    D.Solo.barrier()


def test_librccl_exports_what_the_in_library_merge_binds():
    """renderMultiDevice (mitsuba_amd/csrc/host_multi.h: Rccl::bind) resolves six entry points of librccl with dlopen / dlsym at the first
    multi-GPU render: a missing symbol must be found here, not on the first 8-GPU lease."""
    import ctypes
    lib = None
    for name in ("librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"):
        try:
            lib = ctypes.CDLL(name, mode=ctypes.RTLD_LOCAL)
            break
        except OSError:
            continue
    if lib is None:
        pytest.skip("no librccl on this machine")
    src = open(os.path.join(ROOT, "mitsuba_amd", "csrc", "host_multi.h")).read()
    bind = src[src.index("void bind()"):src.index("void check(ncclResult_t")]
    import re
    names = re.findall(r'sym\("(\w+)"\)', bind)
    assert sorted(names) == sorted(["ncclCommInitAll", "ncclCommDestroy", "ncclReduce", "ncclGroupStart", "ncclGroupEnd", "ncclGetErrorString"]), names
    for n in names:
        assert hasattr(lib, n), "librccl lacks %s" % n


def test_bench_multi_gpu_line_fields():
    """the N > 1 line of bench.py is the metric's config at N x its samples per pixel (weak scaling) and carries the fixed 4K job with its bounded step count and the
    single-GPU rate of the SAME job (static check of the source:
    the run itself needs GPUs -- tests/test_gpu_round2.py::test_bench_two_gpus)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ("single_gpu_same_job", "MULTI_GPU_MAX_STEPS", '"strong" if args.workload else "weak"', "scaling_note"):
        assert key in src, key
    assert "scaling_efficiency" not in src          # (the driver computes efficiencies from the per-N values; the line carries the values and the one-GPU rate of the strong-scaling job)
