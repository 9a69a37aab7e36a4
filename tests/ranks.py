"""Launching the ranks of a data-parallel test, written once.

`run_ranks(worker, world, ...)` spawns `world` fresh processes, each inside `rendezvous(...)`, and returns {rank: what the
worker returned}.  Its contract: ONE deadline for the whole group; the FIRST rank that exits non-zero (assertion, abort,
segmentation fault) stops every other rank at once, so nothing goes on using the device after a peer has died; every child is
reaped before the call returns, whatever happened.  Nothing is retried.

`single_rank_env(...)` is the environment of the tests that run one rank as a plain subprocess."""
import contextlib
import datetime
import multiprocessing.connection
import os
import signal
import socket
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRACE = 10                    # seconds a terminated rank gets before it is killed


def free_port():
    """A port the kernel says is free right now (a pid-derived one can collide with another test process)."""
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


@contextlib.contextmanager
def rendezvous(rank, world, port, backend="gloo", init=None, device=None):
    """Inside a spawned worker: the rendezvous environment, the device, the process group; yields the device string.
    gloo: every rank on cuda:0 (one-GPU box), or on the CPU when there is no GPU or device="cpu"; nccl (= RCCL): one device per
    rank.  init(backend, rank=, world_size=) replaces the default initialisation (a test of the package's own entry point)."""
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    if device is None:
        device = f"cuda:{rank}" if backend == "nccl" else "cuda:0" if torch.cuda.is_available() else "cpu"
    if device != "cpu":
        torch.cuda.set_device(device)
    # short collective timeout: a rank whose peer is gone errors out by itself, should the launcher not get to it first
    if init is not None:
        init(backend, rank=rank, world_size=world)
    elif backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120),
                                device_id=torch.device(device))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    try:
        yield device
    finally:
        dist.destroy_process_group()


def _rank_main(worker, rank, world, port, backend, init, device, ret, args):
    with rendezvous(rank, world, port, backend, init, device) as dev:
        ret[rank] = worker(rank, world, dev, *args)


def _exit_name(code):
    if code is not None and code < 0:
        try:
            return f"{code} ({signal.Signals(-code).name})"
        except ValueError:
            pass
    return str(code)


def run_ranks(worker, world, *args, backend="gloo", timeout=300, init=None, device=None):
    """worker(rank, world, dev, *args), a module-level function (spawn pickles it), once per rank; {rank: its return value}.
    AssertionError naming every rank's exit code if one fails or the group is not done `timeout` seconds from now."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = free_port()
    with ctx.Manager() as manager:
        ret = manager.dict()
        procs = [ctx.Process(target=_rank_main, args=(worker, r, world, port, backend, init, device, ret, args))
                 for r in range(world)]
        for p in procs:
            p.start()
        deadline = time.monotonic() + timeout
        try:
            while True:
                alive = [p for p in procs if p.exitcode is None]
                left = deadline - time.monotonic()
                if not alive or left <= 0 or any(p.exitcode for p in procs):
                    break
                # (a rank that exits between the line above and this one has a ready sentinel: no wait on an empty list)
                multiprocessing.connection.wait([p.sentinel for p in alive], timeout=left)
        finally:                                   # (a KeyboardInterrupt in the wait included) no child outlives the call
            failed = [r for r, p in enumerate(procs) if p.exitcode]
            stopped = [r for r, p in enumerate(procs) if p.exitcode is None]
            for r in stopped:
                procs[r].terminate()
            grace = time.monotonic() + GRACE
            for r in stopped:
                procs[r].join(max(0.0, grace - time.monotonic()))
                if procs[r].exitcode is None:
                    procs[r].kill()
                    procs[r].join()
        out = dict(ret)
    if failed or stopped:
        why = "after the first failure" if failed else f"for the deadline of {timeout} s"
        lines = [f"rank {r}: exit code {_exit_name(p.exitcode)}"
                 + (f", terminated by the launcher {why}" if r in stopped else "") for r, p in enumerate(procs)]
        raise AssertionError(f"{worker.__name__} on {world} {backend} ranks did not complete:\n  " + "\n  ".join(lines))
    return out


def single_rank_env(port=None, **extra):
    """os.environ for ONE rank run as a subprocess: the world-1 rendezvous, the single-rank data-parallel switch, the repository
    on PYTHONPATH, no SDA_ENGINE_* switch inherited; `extra` on top."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SDA_ENGINE_")}
    env.update(SDA_DP_SINGLE_RANK="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port() if port is None else port),
               RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    env.update(extra)
    return env
