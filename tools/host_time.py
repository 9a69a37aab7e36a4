"""Host-side cost of one training step (Python + launch overhead) against its GPU time (diagnostic): is the host far
enough ahead of the GPU that its time never shows?  Per step (bench.py's step): host-only time (enqueue without waiting), the
GPU-drained time, and per phase how long the host takes to enqueue it.    python tools/host_time.py [B=256]"""
import sys
import time

import harness


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    enc, lossf, opt, X, Y, step = harness.headline_step(B=B)
    ph = {n: 0.0 for n in harness.PHASES}
    last = [0.0]

    def phases():                                # the host's clock at every phase boundary
        last[0] = time.perf_counter()

        def mark(name):
            now = time.perf_counter()
            ph[name] += now - last[0]
            last[0] = now
        step(mark=mark)

    for _ in range(8): step()
    harness.settle()
    N = 30
    host, drained = harness.host_clock(phases, N, 0)
    print(f"B={B}: host-only {host:.2f} ms/step, with GPU drain {drained:.2f} ms/step")
    print("host time per phase (ms):", {k: round(1e3 * v / N, 3) for k, v in ph.items()})
    # the same with the GPU idle at every step's start (host latency fully exposed): step time = GPU time + whatever the host adds
    ts = [harness.host_clock(step, 1, 0)[1] for _ in range(10)]
    print(f"one step from an idle GPU: {harness.summarize(ts).median:.2f} ms")


if __name__ == "__main__":
    main()
