"""tests/ranks.py's launcher on CPU gloo ranks: results come back per rank; the first failing rank stops the others long before
they would have finished; a group past its deadline is stopped; no child is left behind."""
import multiprocessing
import os
import time

import pytest
import torch
import torch.distributed as dist

from tests.ranks import run_ranks


def _allreduce(rank, world, dev, base):
    t = torch.full((3,), float(base + rank))
    dist.all_reduce(t)
    return t, dev


def _one_dies(rank, world, dev, how):
    if rank == 1:
        if how == "raise":
            raise RuntimeError("rank 1 gives up")
        os._exit(3)
    time.sleep(120)                       # a peer that would hold the GPU for two minutes before its first collective
    dist.barrier()


def _sleeps(rank, world, dev):
    time.sleep(120)


def test_results_come_back_per_rank():
    out = run_ranks(_allreduce, 2, 10, device="cpu")
    assert sorted(out) == [0, 1]
    for r in (0, 1):
        assert torch.equal(out[r][0], torch.full((3,), 21.0)) and out[r][1] == "cpu"
    assert multiprocessing.active_children() == []


@pytest.mark.parametrize("how,code", [("raise", "1"), ("exit", "3")])
def test_first_failure_stops_the_other_rank(how, code):
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        run_ranks(_one_dies, 2, how, device="cpu")
    took = time.monotonic() - t0
    msg = str(e.value)
    assert f"rank 1: exit code {code}" in msg, msg
    assert "rank 0: exit code -15 (SIGTERM), terminated by the launcher after the first failure" in msg, msg
    assert "terminated" not in msg.split("rank 1:")[1], msg
    assert took < 60, took                # the sleeping rank alone would have held the call for 120 s
    assert multiprocessing.active_children() == []


def test_deadline_stops_every_rank():
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        run_ranks(_sleeps, 2, device="cpu", timeout=5)
    msg = str(e.value)
    for r in (0, 1):
        assert f"rank {r}: exit code -15 (SIGTERM), terminated by the launcher for the deadline of 5 s" in msg, msg
    assert 5 <= time.monotonic() - t0 < 60
    assert multiprocessing.active_children() == []
