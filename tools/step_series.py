"""GPU and host time of EVERY step of a free-running loop (no synchronisation inside; diagnostic): an event after each step's
optimiser launch gives the GPU-side step period, time.perf_counter the host's enqueue time.  Shows periodic slow episodes.
    python tools/step_series.py [N=120] [SETTLE=0]"""
import gc
import os
import sys
import time

import numpy as np
import torch

import harness


def main():
    enc, lossf, opt, X, Y, step = harness.headline_step(training_stream=False)
    # the step's chain on a high-priority stream, as train.py / bench.py run it (speech_decoding_amd/streams.py);
    # SDA_MAIN_PRIO=default keeps torch's default stream, SDA_MAIN_PRIO=0 an explicit normal-priority stream (diagnostic)
    prio = os.environ.get("SDA_MAIN_PRIO", "-1")
    if prio != "default":
        torch.cuda.set_stream(torch.cuda.Stream(priority=int(prio)))
    for _ in range(8): step()
    harness.settle()
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    SETTLE = int(sys.argv[2]) if len(sys.argv) > 2 else 0      # steps between the heap collection and the measured loop (bench.py: 2)
    for _ in range(SETTLE): step()
    if SETTLE: torch.cuda.synchronize()
    evs, host = [], []
    e = harness.timing_event(); e.record(); evs.append(e)      # (periods between steps, not brackets around calls: its own events)
    for _ in range(N):
        t0 = time.perf_counter(); step(); host.append((time.perf_counter() - t0) * 1e3)
        e = harness.timing_event(); e.record(); evs.append(e)
    torch.cuda.synchronize()
    gpu = [evs[i].elapsed_time(evs[i + 1]) for i in range(N)]
    print("gpu :", " ".join(f"{t:.1f}" for t in gpu))
    print("host:", " ".join(f"{t:.1f}" for t in host))
    print(f"gpu median {np.median(gpu):.3f} mean {np.mean(gpu):.3f}; host median {np.median(host):.3f} mean {np.mean(host):.3f}; gc counts {gc.get_count()}")


if __name__ == "__main__":
    main()
