"""Time one training step at the BASELINE.json per-GPU shapes (diagnostic): configs 2, 4, 5."""
import torch

import harness


def run(name, C, S, T, B, dtype="bf16", steps=8):
    enc, lossf, opt, X, Y, step = harness.headline_step(dtype, B, S, C, T)
    ms = harness.host_clock(step, steps, 3)[1]
    print(f"{name}: C={C} S={S} T={T} B={B} {dtype}: {ms:.2f} ms/step, {B/ms*1e3:.0f} seg/s, loss {float(step().detach()):.3f}, "
          f"mem {torch.cuda.max_memory_allocated()/2**30:.1f} GiB", flush=True)


def main():
    run("config2", 208, 27, 360, 256)
    run("config4/GPU", 60, 1, 360, 512)
    run("config5/GPU", 306, 100, 1000, 512)


if __name__ == "__main__":
    main()
