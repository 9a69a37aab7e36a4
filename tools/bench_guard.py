"""The gradient guard measured on the GPU, at BASELINE config 2 (208 channels, 27 subjects, 360 samples, batch 256).
Diagnostic; not part of the product.

    python tools/bench_guard.py [--json profiles/guard_bench.json] [--iters 200] [--reps 7] [--steps 20]

1. The three launches alone over the real encoder's parameter list (+ the loss temperature), by device events after warm-up:
   microseconds and the bytes each must move.  In the same run, for comparison: sda_adam_multi alone, and the host guard
   (torch._amp_foreach_non_finite_check_and_unscale_ + .item(), a host clock around it: it ends in a synchronisation).
2. The fp16 training step (forward, loss, backward, guard, Adam; train.py's two step builders): the host guard
   (make_backward_and_step + FusedAdam + LossScaler) against the device guard (make_guarded_step + GuardedAdam), alternating,
   `reps` windows of `steps` steps each; medians and the spread (max - min over the windows) the run itself shows.
3. bf16 with max_grad_norm=1 against bf16 without (the cost of clipping where there is no guard to replace).
Prints the table DESIGN.md §7 quotes and writes the JSON."""
import argparse
import os
import sys

import numpy as np
import torch

import harness

C, S, T, B, F = 208, 27, 360, 256, 1024


def timeit(fn, iters):
    return harness.us(harness.window(fn, iters, 10))          # us per call


def host_timeit(fn, iters):
    """for a call that ends in a host synchronisation: a host clock around it"""
    return harness.us(harness.host_clock(fn, iters, 10)[1])


def launches_alone(dev, iters):
    from speech_decoding_amd import lib as L, ops
    from speech_decoding_amd.optim import _real, adam_table
    _, _, _, params = harness.headline_modules("fp16")
    g = torch.Generator(device=dev).manual_seed(1)
    items = []
    for p in params:
        p.grad = torch.view_as_complex(torch.randn(*p.shape, 2, generator=g, device=dev) * 1e-3) if p.is_complex() \
            else torch.randn(p.shape, generator=g, device=dev) * 1e-3
        items.append((_real(p.data), _real(p.grad), torch.zeros_like(_real(p.data)), torch.zeros_like(_real(p.data))))
    raw, max_n = adam_table(items)
    n, N = len(items), sum(it[0].numel() for it in items)
    table = ops.upload_small(raw, dev)
    parts = torch.empty(ops.grad_guard_parts(n, max_n), dtype=torch.float64, device=dev)
    gx = parts.numel() // (2 * n)
    state = torch.zeros(L.GUARD_STATE, dtype=torch.float64, device=dev)
    state[L.GUARD_SCALE] = 1.0
    st = torch.cuda.current_stream().cuda_stream
    lib = L.load()
    rows = []

    def row(name, us, nbytes, note=""):
        rows.append(dict(what=name, us=round(us, 2), MB=round(nbytes / 1e6, 3), TBps=round(nbytes / us / 1e6, 3), note=note))

    row("sda_grad_sumsq_multi", timeit(lambda: ops.grad_sumsq_multi(table, n, max_n, parts), iters), 4 * N + 8 * parts.numel())
    row("sda_grad_guard_finish", timeit(lambda: ops.grad_guard_finish(parts, n, gx, state, 0.0, 0.9, 0.999, 2000, 2.0 ** 24, False), iters),
        8 * parts.numel())
    row("sda_adam_multi_guarded", timeit(lambda: ops.adam_multi_guarded(table, n, max_n, 1e-4, 0.9, 0.999, 1e-8, state), iters), 28 * N)

    def three():
        ops.grad_sumsq_multi(table, n, max_n, parts)
        ops.grad_guard_finish(parts, n, gx, state, 1.0, 0.9, 0.999, 2000, 2.0 ** 24, False)
        ops.adam_multi_guarded(table, n, max_n, 1e-4, 0.9, 0.999, 1e-8, state)
    row("the three launches back to back", timeit(three, iters), 32 * N + 16 * parts.numel())
    row("sda_adam_multi", timeit(lambda: L.check(lib.sda_adam_multi(table.data_ptr(), n, max_n, 1e-4, 0.9, 0.999, 1e-8, 7, st)), iters), 28 * N)
    grads = [it[1] for it in items]
    found, inv = torch.zeros(1, device=dev), torch.ones(1, device=dev)

    def host_guard():
        found.zero_()
        torch._amp_foreach_non_finite_check_and_unscale_(grads, found, inv)
        return bool(found.item())
    row("host guard: torch check-and-unscale + .item()", host_timeit(host_guard, iters), 8 * N, "host clock; idle GPU, so the .item() waits only for its own launch")
    row("torch check-and-unscale alone", timeit(lambda: torch._amp_foreach_non_finite_check_and_unscale_(grads, found, inv), iters), 8 * N)
    return dict(tensors=n, elements=N, grid=[gx, n], partial_doubles=parts.numel(), rows=rows)


class Loop:
    def __init__(self, dtype, guarded, max_grad_norm, dev, pool):
        import train
        from speech_decoding_amd.amp import LossScaler
        from speech_decoding_amd.optim import FusedAdam, GuardedAdam
        cfg, self.enc, self.lossf, params = harness.headline_modules(dtype)
        scaler = LossScaler.for_dtype(self.enc.compute_dtype, global_batch=B, T=T)
        if guarded:
            self.opt = GuardedAdam(params, lr=float(cfg.lr), max_grad_norm=max_grad_norm, loss_scale=scaler.scale_value,
                                   dynamic=scaler.enabled, growth_interval=scaler.growth_interval, max_scale=scaler.max_scale)
            self.step = train.make_guarded_step(self.enc, self.lossf, params, self.opt, 1, dev)
        else:
            self.opt = FusedAdam(params, lr=float(cfg.lr))
            self.step = train.make_backward_and_step(self.enc, self.lossf, params, self.opt, scaler, 1, dev)
        self.pool, self.i = pool, 0
        self.rng = np.random.RandomState(100)

    def one(self):
        """train.py's step: its own step builders behind the headline forward, no retrieval ranks"""
        X, Y = self.pool[self.i % len(self.pool)]
        self.i += 1
        subj = torch.from_numpy(self.rng.randint(0, S, size=B).astype(np.int32))
        self.lossf.prefetch(Y, self.enc.compute_dtype)
        loss = self.lossf(Y, self.enc(X, subj))
        self.step(loss)

    def run(self, n):
        """n steps; host ms per step to enqueue them, wall ms per step until the device is done"""
        return harness.host_clock(self.one, n, 0)


def alternate(names, loops, reps, steps, warm=12):
    for lp in loops:
        lp.run(warm)
    wall = {n: [] for n in names}
    host = {n: [] for n in names}
    for _ in range(reps):
        for n, lp in zip(names, loops):
            h, w = lp.run(steps)
            host[n].append(h)
            wall[n].append(w)
    out = {}
    for n in names:
        w = harness.summarize(wall[n])
        out[n] = dict(step_ms_median=round(w.median, 4), step_ms_min=round(w.min, 4), step_ms_max=round(w.max, 4),
                      spread_ms=round(w.max - w.min, 4), host_enqueue_ms_median=round(harness.summarize(host[n]).median, 4),
                      windows_ms=[round(x, 4) for x in wall[n]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join("profiles", "guard_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("bench_guard.py: at least five repetitions of each path")
    harness.need_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = dict(shape=dict(C=C, S=S, T=T, batch=B, F=F), device=torch.cuda.get_device_name(0), iters=a.iters, reps=a.reps, steps=a.steps)
    out["launches"] = launches_alone(dev, a.iters)
    pool = [harness.headline_batch(B, C, T, F, seed=i) for i in range(4)]
    import gc
    for key, dtype, names, specs in (("fp16_step", "fp16", ("host guard", "device guard"), ((False, None), (True, None))),
                                     ("bf16_step", "bf16", ("no clipping", "max_grad_norm=1"), ((False, None), (True, 1.0)))):
        loops = [Loop(dtype, guarded, mgn, dev, pool) for guarded, mgn in specs]
        out[key] = alternate(names, loops, a.reps, a.steps)
        g = loops[1].opt
        out[key]["guarded_state"] = dict(steps_taken=g.steps_taken, skipped_steps=g.skipped_steps, loss_scale=g.loss_scale,
                                         last_grad_norm=g.last_grad_norm, last_coef=g.last_coef)
        del loops, g
        gc.collect()
        torch.cuda.empty_cache()
    h, d = out["fp16_step"]["host guard"], out["fp16_step"]["device guard"]
    spread = max(h["spread_ms"], d["spread_ms"])
    out["fp16_step"]["device_minus_host_ms"] = round(d["step_ms_median"] - h["step_ms_median"], 4)
    out["fp16_step"]["within_spread"] = bool(d["step_ms_median"] - h["step_ms_median"] <= spread)
    print("| launch (config 2 parameter list: %d tensors, %.2f M elements) | us | MB moved | TB/s |" % (out["launches"]["tensors"], out["launches"]["elements"] / 1e6))
    print("|---|---|---|---|")
    for r in out["launches"]["rows"]:
        print(f"| {r['what']} | {r['us']:.1f} | {r['MB']:.2f} | {r['TBps']:.2f} |")
    print()
    print("| step at config 2 shapes | median ms | min .. max over the windows | host enqueue ms |")
    print("|---|---|---|---|")
    for key in ("fp16_step", "bf16_step"):
        for n, r in out[key].items():
            if isinstance(r, dict) and "step_ms_median" in r:
                print(f"| {key[:4]}, {n} | {r['step_ms_median']:.3f} | {r['step_ms_min']:.3f} .. {r['step_ms_max']:.3f} | {r['host_enqueue_ms_median']:.3f} |")
    print(f"fp16: device - host = {out['fp16_step']['device_minus_host_ms']:+.3f} ms, spread {spread:.3f} ms, within spread: {out['fp16_step']['within_spread']}")
    harness.emit(out, a.json)


if __name__ == "__main__":
    main()
