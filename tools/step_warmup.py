"""Wall time of each of the first N config-2 training steps (synchronised per step): where does warm-up end? (diagnostic)
    python tools/step_warmup.py [N=40] [engine_attribute=literal | gc=True|False ...]"""
import gc
import sys

import torch

import harness


def main():
    enc, lossf, opt, X, Y, step = harness.headline_step()
    for kv in sys.argv[2:]:
        k, v = kv.split("=")
        if k == "gc":
            (gc.enable if eval(v) else gc.disable)()
            continue
        setattr(enc.engine, k, eval(v))
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    ts = [harness.host_clock(step, 1, 0)[1] for _ in range(n)]          # no warm-up: the first steps are what is asked about
    print(" ".join(f"{t:.1f}" for t in ts))
    print("allocator:", {k: v for k, v in torch.cuda.memory_stats().items() if k in ("num_alloc_retries", "num_device_alloc", "num_device_free")})


if __name__ == "__main__":
    main()
