"""How every tool under tools/ measures: the repository on the import path, the GPU requirement, the four timing forms, one
summary of a sample list, the training step bench.py times, one child process under a time limit, one JSON line out.

Times are milliseconds per call; `us()` converts for the tools that print microseconds.  The clock (event source, device
synchronisation, host clock) is a parameter of every timing form, the device's by default: a CPU test passes a stub."""
import contextlib
import gc
import json
import os
import statistics
import subprocess
import sys
import time
import types
import warnings
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def need_gpu():
    """A measurement without the GPU is an error, never a CPU number."""
    if not torch.cuda.is_available():
        raise RuntimeError("this tool measures on the GPU and none is available: nothing is measured without one")


def timing_event():
    """A device event that records times; for the tools that bracket something other than a call (step periods, phases)."""
    return torch.cuda.Event(enable_timing=True)


GPU_CLOCK = types.SimpleNamespace(event=timing_event, sync=lambda: torch.cuda.synchronize(), now=time.perf_counter)


# ------------------------------------------------------------------------------------------------------ the timing forms
def rounds(fn, iters, windows, warmup, clock=GPU_CLOCK, stream=None):
    """`windows` windows after `warmup` calls, each one event pair around `iters` calls: [ms per call of every window].
    `stream`: issue the calls (and record the events) on this stream instead of the current one."""
    if clock is GPU_CLOCK:
        need_gpu()
    with contextlib.nullcontext() if stream is None else torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        clock.sync()
        out = []
        for _ in range(windows):
            e0, e1 = clock.event(), clock.event()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            clock.sync()
            out.append(e0.elapsed_time(e1) / iters)
    return out


def window(fn, iters, warmup, clock=GPU_CLOCK, stream=None):
    """One event pair around `iters` calls after `warmup` calls: ms per call."""
    return rounds(fn, iters, 1, warmup, clock, stream)[0]


def alternating(fns, iters, warmup, reps=1, sync_each=True, clock=GPU_CLOCK):
    """Every callable between its own event pair, `reps` back-to-back calls per pair, the callables taking turns inside each of
    the `iters` iterations, after `warmup` rounds of all of them: one list of `iters` samples (ms per call) per callable.
    sync_each: wait for every bracket before the next call, so that each call starts on an idle GPU; False keeps the GPU fed
    and reads the events at the end."""
    if clock is GPU_CLOCK:
        need_gpu()
    for _ in range(warmup):
        for f in fns:
            f()
    clock.sync()
    samples, pending = [[] for _ in fns], []
    for _ in range(iters):
        for i, f in enumerate(fns):
            e0, e1 = clock.event(), clock.event()
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            if sync_each:
                e1.synchronize()
                samples[i].append(e0.elapsed_time(e1) / reps)
            else:
                pending.append((i, e0, e1))
    clock.sync()
    for i, e0, e1 in pending:
        samples[i].append(e0.elapsed_time(e1) / reps)
    return samples


def host_clock(fn, iters, warmup, clock=GPU_CLOCK):
    """The host's clock around `iters` calls that end in a device synchronisation, after `warmup` calls:
    (ms per call until the last call returned: the host's enqueue time, ms per call until the device was done)."""
    if clock is GPU_CLOCK:
        need_gpu()
    for _ in range(warmup):
        fn()
    clock.sync()
    t0 = clock.now()
    for _ in range(iters):
        fn()
    t1 = clock.now()
    clock.sync()
    return (t1 - t0) / iters * 1e3, (clock.now() - t0) / iters * 1e3


# ------------------------------------------------------------------------------------------------------------- summaries
class Summary(NamedTuple):
    n: int
    mean: float
    median: float
    min: float
    max: float


def summarize(samples):
    return Summary(len(samples), statistics.fmean(samples), statistics.median(samples), min(samples), max(samples))


def us(ms):
    """milliseconds (a number or a Summary) as microseconds"""
    return Summary(ms.n, *(1e3 * v for v in ms[1:])) if isinstance(ms, Summary) else 1e3 * ms


# --------------------------------------------------------------------------------------------------- the headline step
def headline_modules(dtype="bf16", S=27, C=208, F=1024, seed=0):
    """The models bench.py trains: (cfg, BrainEncoder, CLIPLoss, their parameters), on the current device, in training mode."""
    need_gpu()
    from speech_decoding_amd import BrainEncoder, CLIPLoss, load_config
    from speech_decoding_amd.layout import synthetic_positions
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(seed)
    np.random.seed(seed)
    overrides = [f"num_subjects={S}", f"compute_dtype={dtype}", "dataset=Gwilliams2022"]
    if F != 1024:                                   # (last4layers, the default, means F = 1024 whatever F says)
        overrides += [f"F={F}", "preprocs.last4layers=False"]
    cfg = load_config(overrides=overrides)
    cfg["sensor_positions"] = synthetic_positions(C, 0).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = BrainEncoder(cfg).to(dev).train()
    lossf = CLIPLoss(cfg).to(dev).train()
    return cfg, enc, lossf, list(enc.parameters()) + list(lossf.parameters())


def headline_batch(B=256, C=208, T=360, F=1024, seed=0):
    """One batch of bench.py's synthetic pool, resident: X ~ N(0, 1) clamped to +-20, Y = P X + 0.5 eps."""
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(1234 + seed)
    Pm = torch.randn(F, C, generator=torch.Generator().manual_seed(7)).to(dev) / np.sqrt(C)
    X = torch.randn(B, C, T, generator=g, device=dev).clamp_(-20, 20)
    Y = torch.einsum("fc,bct->bft", Pm, X) + 0.5 * torch.randn(B, F, T, generator=g, device=dev)
    return X, Y.contiguous()


PHASES = ("prefetch", "enc_fwd", "loss", "ranks", "backward", "adam")


def headline_step(dtype="bf16", B=256, S=27, C=208, T=360, F=1024, seed=0, training_stream=True):
    """The training step bench.py times, at its defaults the headline configuration: (enc, lossf, opt, X, Y, step).
    step(subj=None, mark=None) runs prefetch, forward, loss, retrieval_ranks, zero_grad, backward, FusedAdam and returns the
    loss; the subject indices are drawn fresh every step unless given; mark(name) is called after each of PHASES.
    training_stream: make the high-priority stream current, as bench.py and train.py do; a tool that picks the stream
    itself passes False."""
    from speech_decoding_amd import loss as sda_loss
    from speech_decoding_amd.amp import LossScaler
    from speech_decoding_amd.optim import FusedAdam
    from speech_decoding_amd.streams import use_training_stream
    cfg, enc, lossf, params = headline_modules(dtype, S, C, F, seed)
    if training_stream:
        use_training_stream()
    opt = FusedAdam(params, lr=float(cfg.lr))
    scaler = LossScaler.for_dtype(enc.compute_dtype, global_batch=B, T=T)      # fp16: static scale; bf16 / fp32: a no-op
    X, Y = headline_batch(B, C, T, F, seed)
    rng = np.random.RandomState(100 + seed)
    one = torch.ones((), dtype=torch.float32, device=X.device)

    def step(subj=None, mark=None):
        mark = mark or (lambda name: None)
        if subj is None:
            subj = torch.from_numpy(rng.randint(0, S, size=B).astype(np.int32))
        lossf.prefetch(Y, enc.compute_dtype)
        mark("prefetch")
        Z = enc(X, subj)
        mark("enc_fwd")
        loss = lossf(Y, Z)
        mark("loss")
        sda_loss.retrieval_ranks(Y, Z)
        mark("ranks")
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward(gradient=one)
        scaler.unscale_(params)
        mark("backward")
        opt.step()
        mark("adam")
        return loss

    return enc, lossf, opt, X, Y, step


def settle():
    """After warm-up, as bench.py: drain the device, collect the heap and freeze it (a generation-2 collection inside a timed
    region is worth 80 ms)."""
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()


# ------------------------------------------------------------------------------------------------ children and records
TIME_LIMIT = 124          # run_child's status for a child ended at its time limit (what timeout(1) returns)


def run_child(argv, limit, lines=None):
    """One child process under a time limit of `limit` seconds: its exit status, TIME_LIMIT if it had to be ended.  `lines`: a
    list that receives the child's standard output line by line (otherwise it goes where the parent's goes).  A sweep that
    gives every size a fresh process ends at the first status that is not 0: nothing is started after a child ended badly."""
    try:
        done = subprocess.run(argv, timeout=limit, stdout=None if lines is None else subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        return TIME_LIMIT
    if lines is not None:
        lines.extend(done.stdout.splitlines())
    return done.returncode


def child_error(status, limit):
    return f"time limit of {limit} s" if status == TIME_LIMIT else f"exit status {status}"


def rounded(v, digits):
    if isinstance(v, float):
        return round(v, digits)
    if isinstance(v, dict):
        return {k: rounded(x, digits) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [rounded(x, digits) for x in v]
    return v


def emit(record, out=None, append=False, digits=None):
    """One JSON line on standard output, floats rounded to `digits` if given; with `out` the record also goes into that
    file: as one more line (append) or as the file's whole, indented content."""
    if digits is not None:
        record = rounded(record, digits)
    print(json.dumps(record), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a" if append else "w") as f:
            f.write(json.dumps(record) + "\n" if append else json.dumps(record, indent=1) + "\n")
