"""A/B of engine switches on the config-2 training step in ONE process, interleaved rounds (box-to-box and run-to-run
variance is larger than most of the effects being compared).  Usage: python tools/ab_step.py [rounds] [name:attr=value,...]"""
import sys

import numpy as np
import torch

import harness


def main():
    # (this tool picks the stream the step is issued on: the pseudo-attribute main_priority below)
    enc, lossf, opt, X, Y, step = harness.headline_step(training_stream=False)
    # variants: name:attr=value,attr=value ... (or ';' between the pairs when a value contains a comma) (engine attributes; values are Python literals)
    specs = sys.argv[2:] or ["base:", "flat_fwd_off:flat_tiles_forward=False"]
    variants = {}
    for spec in specs:
        name, _, rest = spec.partition(":")
        variants[name] = {kv.split("=")[0]: eval(kv.split("=")[1]) for kv in rest.split(";" if ";" in rest else ",") if kv}
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    eng = enc.engine
    eng.main_priority = 0                   # pseudo-attribute of this tool: priority of the stream the step is issued on
    defaults = {k: getattr(eng, k) for v in variants.values() for k in v}
    streams = {0: torch.cuda.current_stream(), -1: torch.cuda.Stream(priority=-1)}

    def apply(v):
        for k, d in defaults.items(): setattr(eng, k, d)
        for k, x in v.items(): setattr(eng, k, x)
        eng._seg_cache.clear()
        eng._side.clear()

    res = {k: [] for k in variants}
    for k, v in variants.items():           # warm-up of every variant (workspaces, attribute calls)
        apply(v)
        with torch.cuda.stream(streams[eng.main_priority]):
            for _ in range(3): step()
        torch.cuda.synchronize()
    harness.settle()
    for r in range(rounds):
        for k, v in variants.items():
            apply(v)
            with torch.cuda.stream(streams[eng.main_priority]):
                res[k].append(harness.host_clock(step, 10, 0)[1])
    for k, v in res.items():
        print(f"{k:10s} median {np.median(v):.3f} ms  min {min(v):.3f}  all {[round(x, 3) for x in v]}")


if __name__ == "__main__":
    main()
