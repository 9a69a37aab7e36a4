"""How long does the main stream sit idle at each cross-stream wait of a config-2 training step?  (diagnostic)
Also reports the main stream's total idle time per step: step wall time minus the sum of event-bracketed segments is not
available without a trace, so the waits are the part that scheduling can change."""
import numpy as np

import harness


def main():
    enc, lossf, opt, X, Y, step = harness.headline_step()
    marks = []

    def marked():                                # (wait and phase brackets, not brackets around calls: its own events)
        ev = [harness.timing_event()]
        ev[0].record()

        def mark(name):
            if name != "loss":                   # loss + ranks are one phase here
                ev.append(harness.timing_event())
                ev[-1].record()
        step(mark=mark)
        marks.append(ev)

    for _ in range(5): step()
    harness.GPU_CLOCK.sync()
    enc.engine.probe = []
    n = 20
    wall = harness.host_clock(marked, n, 0)[1]
    by = {}
    for label, e0, e1 in enc.engine.probe:
        by.setdefault(label, []).append(e0.elapsed_time(e1) * 1e3)
    print(f"step {wall:.3f} ms (with probes)")
    for k, v in by.items():
        print(f"  wait '{k}': {len(v) / n:.0f} per step, mean {np.mean(v):7.1f} us, median {np.median(v):7.1f}, max {np.max(v):7.1f}")
    ph = np.array([[m[i].elapsed_time(m[i + 1]) * 1e3 for i in range(5)] for m in marks])
    gap = np.array([marks[i][5].elapsed_time(marks[i + 1][0]) * 1e3 for i in range(len(marks) - 1)])
    print("  main-stream phases (us, median): prefetch %.0f  forward %.0f  loss+ranks %.0f  backward %.0f  adam %.0f  | between steps %.0f" %
          (*np.median(ph, axis=0), np.median(gap)))


if __name__ == "__main__":
    main()
