"""What-if (timing only, results are NOT checked): the config-2 training step captured into ONE HIP graph and replayed,
against the same step launched eagerly, interleaved in one process.  The naive capture bakes the subject indices and
Adam's step count into the graph, so its numbers are wrong after the first replay — only its duration means anything.
Usage: python tools/graph_probe.py [rounds]"""
import sys
import traceback

import numpy as np
import torch

import harness


def main():
    enc, lossf, opt, X, Y, step = harness.headline_step(training_stream=False)      # (captured from torch's default stream)
    enc.set_drop_centre(3)
    for _ in range(8): step()
    harness.settle()
    fixed = torch.from_numpy(np.random.RandomState(0).randint(0, enc.num_subjects, size=X.shape[0]).astype(np.int32))
    graph = torch.cuda.CUDAGraph()
    try:
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph):
            step(fixed)
        torch.cuda.synchronize()
        ok = True
    except Exception:                                        # noqa: BLE001
        traceback.print_exc()
        ok = False
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    res = {"eager": [], "graph": []}
    for r in range(rounds):
        res["eager"].append(harness.host_clock(step, 20, 0)[1])
        if ok:
            res["graph"].append(harness.host_clock(graph.replay, 20, 0)[1])
    for k, v in res.items():
        if v:
            print(f"{k:6s} median {np.median(v):.3f} ms  min {min(v):.3f}  all {[round(x, 3) for x in v]}")


if __name__ == "__main__":
    main()
