"""Per-phase GPU time of one training step (diagnostic): prefetch / encoder fwd / loss fwd / ranks / backward / Adam, the device
drained at every phase boundary.    python tools/phase_time.py [bf16|fp16|fp32]"""
import sys

import torch

import harness


def main():
    dtype = sys.argv[1] if len(sys.argv) > 1 else "bf16"
    enc, lossf, opt, X, Y, step = harness.headline_step(dtype)
    acc = {n: 0.0 for n in harness.PHASES}
    N = 20
    for it in range(5 + N):
        torch.cuda.synchronize()
        e = [harness.timing_event()]
        e[0].record()

        def mark(name):                          # (phase brackets, not brackets around calls: its own events)
            torch.cuda.synchronize()
            e.append(harness.timing_event())
            e[-1].record()
        step(mark=mark)
        torch.cuda.synchronize()
        if it >= 5:
            for i, n in enumerate(harness.PHASES):
                acc[n] += e[i].elapsed_time(e[i + 1])
    print(dtype, {n: round(v / N, 3) for n, v in acc.items()}, "sum", round(sum(acc.values()) / N, 3))


if __name__ == "__main__":
    main()
