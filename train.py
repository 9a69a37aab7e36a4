#!/usr/bin/env python3
"""Training / evaluation driver for the MI355X build — same CLI surface and printed scalars as the
reference's `train.py`, own implementation.

    python train.py                          # configs/config.yaml
    python train.py dataset=Brennan2018 batch_size=64 epochs=3 compute_dtype=bf16
    python -m torch.distributed.run --nproc-per-node 8 train.py batch_size=256      # data parallel

What is kept from the reference loop (train.py:148-259):
  * models: BrainEncoder + Classifier + CLIPLoss, Adam over encoder parameters and the loss temperature;
    `loss=mse` trains on MSELoss instead (the reference's regression objective; Adam over the encoder alone),
    `loss=sigmoid` on SigmoidLoss (the pairwise sigmoid contrastive loss; Adam over the encoder, its temperature and its bias);
  * per batch: Z = encoder(X, subject_idxs); loss = CLIPLoss(Y, Z); top-1/top-10 from Classifier(Z, Y);
  * update cadence: Gwilliams2022 steps on every batch, Brennan2018 ONCE per epoch with the last batch's
    loss (train.py:200-209);
  * evaluation in eval() mode on the whole test split as ONE batch (train.py:99,211-233);
  * the per-epoch print line and the optional W&B scalar names; `model_last.pt` = encoder.state_dict().
`data=continuous` (with dataset=Brennan2018) runs that dataset's own input path on the GPU: whole-recording robust scaling
(preprocs.subject_wise), clamp, segment gather with baseline correction (speech_decoding_amd.data.ResidentSubjectFeed).
`data=tracks` (with dataset=Gwilliams2022, compute_dtype=bf16 or fp16) is `data=resident` with the speech embeddings kept as one
resident track per task: a batch's Y is the windows at the segments' onsets, gathered into the loss's operand by one kernel.
What is not: the M/EEG + wav2vec2 dataset classes (they need the raw recordings and un-downloadable weights; their
signal conditioning — band-pass, audio and FFT resampling — is built as speech_decoding_amd.signal_prep, but this
script does not read raw files).  `--data synthetic` (default) builds a seeded stand-in with the same tensor
shapes; a real dataset object can be passed to `run()` as (train_batches, test_batch) callables.

Layout: `build_data` makes the synthetic data of a `data=` kind (the feed, or None for the pool, and the two callables; sampler,
epoch seed and test shard are written there once), `make_backward_and_step` the update, `run` the loop around them.
`max_grad_norm=1.0` clips the gradients by their global norm and `fp16_guard=device` moves fp16's overflow guard off the host;
either one runs the step through `make_guarded_step` (GuardedAdam: norm, guard, clipping and Adam on the device, no read-back).
`clip_duplicates=positive|mask` (default `ignore`: the reference's loss) hands the feed's speech ids to the loss and the
accuracies: the sampler draws with replacement, so a batch can hold one speech segment twice under two brain recordings, and the
repeat then counts as a further positive (or as no negative) instead of a wrong answer.
`clip_negatives=N` (default 0; data=tracks with loss=clip) contrasts every brain segment against N further speech windows per step,
drawn from the training split's resident tracks and read in place (CLIPLoss.forward's `negatives`); evaluation is unchanged.
"""
from __future__ import annotations

import os
import sys
import time
from typing import Callable, Iterable, Optional, Tuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from speech_decoding.models import BrainEncoder, Classifier       # noqa: E402  (train.py:22 import path)
from speech_decoding.utils.loss import CLIPLoss, MSELoss, SigmoidLoss    # noqa: E402  (train.py:24)
from speech_decoding_amd import data as D                          # noqa: E402  (feeds are looked up in the module when run() is called)
from speech_decoding_amd import load_config                        # noqa: E402
from speech_decoding_amd.distributed import allreduce_gradients, broadcast_parameters, shard_range  # noqa: E402
from speech_decoding_amd.loss import speech_labels                 # noqa: E402
from speech_decoding_amd.models import resolve_dtype               # noqa: E402


class SyntheticSegments:
    """Seeded stand-in for the segmented datasets: X (N, C, T) ~ N(0,1) clamped to ±clamp_lim with the first
    baseline samples' mean removed (preproc_utils.py:69-90,128-142), Y = P·X + 0.5·eps (so retrieval is
    learnable), subject indices uniform.  Split by `split_ratio` like the shallow split."""

    def __init__(self, args, n_segments: int, device, seed: int = 0):
        C, T, nb, F, S = D.segment_dims(args)
        g = torch.Generator().manual_seed(seed)
        X = torch.randn(n_segments, C, T, generator=g)
        X = X - X[:, :, :nb].mean(dim=-1, keepdim=True)
        if args.preprocs["clamp"]:
            X = X.clamp(-float(args.preprocs["clamp_lim"]), float(args.preprocs["clamp_lim"]))
        P = torch.randn(F, C, generator=g) / np.sqrt(C)
        Y = torch.einsum("fc,nct->nft", P, X) + 0.5 * torch.randn(n_segments, F, T, generator=g)
        self.X, self.Y = X.to(device), Y.to(device)
        self.subj = torch.randint(0, S, (n_segments,), generator=g, dtype=torch.int32)
        n_train = int(n_segments * float(args.split_ratio))
        self.train_idx = torch.arange(n_train)
        self.test_idx = torch.arange(n_train, n_segments)
        self.gen = torch.Generator().manual_seed(seed + 1)

    def train_batches(self, batch_size: int, updates: int) -> Iterable[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """`updates` batches; like RandomSampler(replacement=True) over the train split (get_dataloaders.py:48-87)
        but without duplicates inside a batch (train.py:181-183 aborts on duplicate segments)."""
        for _ in range(updates):
            pick = self.train_idx[torch.randperm(len(self.train_idx), generator=self.gen)[:batch_size]]
            yield self.X[pick], self.Y[pick], self.subj[pick]

    def test_batch(self):
        i = self.test_idx
        return self.X[i], self.Y[i], self.subj[i]


def build_data(args, data_kind: str, device, rank: int, world: int, with_ids: bool = False, negatives: int = 0):
    """The synthetic data of a `data=` kind -> (feed, train_batches, test_batch).  `feed` is None for the pool; otherwise the
    callables hand out THIS rank's shard of every batch, and feed.pack_embeddings is the caller's to call once the encoder's
    compute dtype is known.  `with_ids`: a feed's batches are the 4-tuples (X, Y, subject_idxs, chunkIDs) with the segments'
    speech ids (the pool draws without repeats and has none to give).  `negatives` (data=tracks): every training batch ends with
    a WindowBank of that many further speech windows of the TRAINING split, none of which carries the speech of a segment of the
    global batch (feed.draw_negatives: the same draw on every rank); the test batch has none.

    data=pool (default): a resident pool of ready-made segments, every rank slicing its shard out of the global batch;
    data=resident: the reference's own input path on the GPU — recordings resident in HBM, RandomSampler(replacement=True)
    (get_dataloaders.py:48-87) cut into rank shards so that no rank materialises another rank's samples, window gather +
    baseline correction + robust scaling + clamp (gwilliams2022.py:129-142,640-661) as one kernel per batch;
    data=continuous (dataset=Brennan2018): that dataset's own input path — the (subjects, channels, time) recording of one
    stimulus resident in HBM, robust scaling + clamp over the WHOLE recording once (preprocs.subject_wise: per subject, or all
    subjects pooled), a batch = chunk i of a random subject with its baseline removed (brennan2018.py:72-152);
    data=tracks (dataset=Gwilliams2022): data=resident with the speech side held the way the reference first computes it — one
    embedding track per task, resident once in the encoder's 16-bit compute dtype (retrieval.WindowBank), a segment = the window
    at its onset; a batch's Y is gathered from the tracks into the loss's packed operand by one kernel (sda_gather_windows), no
    window is materialised.  Same sampler, epoch seeds and evaluation shards as data=resident; compute_dtype=fp32 is refused."""
    batch_size = int(args.batch_size)
    n_seg = int(args.get("synthetic_segments", 4 * batch_size))
    if data_kind == "tracks":
        feed, train_idx, test_idx = D.synthetic_track_dataset(args, device, n_segments=n_seg, dtype=resolve_dtype(args), seed=1234)
    elif data_kind == "resident":
        feed, train_idx, test_idx = D.synthetic_resident_dataset(args, device, n_segments=n_seg, seed=1234)
    elif data_kind == "continuous":
        pre = args.preprocs
        rate = pre["brain_resample_rate"]
        seq = D.segment_dims(args).T
        shift_ms = pre.get("shift_len", 150) if pre.get("shift_brain", True) else 0
        Xc, Yc = D.synthetic_subject_dataset(args, device, length=n_seg * seq + int(rate * (shift_ms / 1000)) + seq // 3, seed=1234)
        feed = D.ResidentSubjectFeed(Xc, Yc, srate=rate, seq_len_sec=pre["seq_len_sec"], baseline_len_sec=pre["baseline_len_sec"],
                                     clamp_lim=float(pre["clamp_lim"]), clamp=bool(pre["clamp"]),
                                     subject_wise=bool(pre.get("subject_wise", True)), shift_ms=shift_ms, seed=1234 + 17)
        del Xc, Yc
        n_train = int(len(feed) * float(args.split_ratio))
        perm = np.random.RandomState(1234).permutation(len(feed))
        train_idx, test_idx = perm[:n_train], perm[n_train:]
    else:
        pool = SyntheticSegments(args, n_seg, device, seed=1234)
        updates = int(args.get("updates_per_epoch", max(1, len(pool.train_idx) // batch_size)))
        return None, lambda: pool.train_batches(batch_size, updates), pool.test_batch
    updates = int(args.get("updates_per_epoch", max(1, len(train_idx) // batch_size)))
    epoch_no = [0]

    def sampler_seed(epoch: int) -> int:
        return 4321 + epoch

    def train_batches():
        sampler = D.ShardedRandomSampler(len(train_idx), batch_size, updates, rank, world, seed=sampler_seed(epoch_no[0]))
        epoch_no[0] += 1
        # (under data parallelism the draws for the whole global batch are made on every rank alike and sliced)
        if not negatives:
            yield from feed.batches(sampler, index_map=train_idx, with_ids=with_ids)
            return
        # the global batches once more, from a twin of the sampler: every rank excludes the WHOLE batch's speech and draws alike
        twin = D.ShardedRandomSampler(len(train_idx), batch_size, updates, rank, world, seed=sampler_seed(epoch_no[0] - 1))
        for out, gidx in zip(feed.batches(sampler, index_map=train_idx, with_ids=with_ids), twin.global_batches()):
            yield (*out, feed.speech_bank(feed.draw_negatives(negatives, np.asarray(train_idx)[gidx.numpy()], train_idx)))

    def test_batch():
        lo, hi = shard_range(len(test_idx), rank, world)
        out = feed.batch(test_idx[lo:hi])
        return (*out, torch.from_numpy(feed.speech_ids(test_idx[lo:hi]))) if with_ids else out
    return feed, train_batches, test_batch


def make_backward_and_step(brain_encoder, loss_func, params, optimizer, scaler, world: int, device):
    """backward_and_step(loss) for the loop: backward of the scaled loss, the gradient all-reduce under data parallelism, fp16's
    overflow guard, Adam."""
    clip = isinstance(loss_func, (CLIPLoss, SigmoidLoss))   # a contrastive loss: it has parameters of its own
    fp16 = scaler.enabled            # (not `scale != 1`: a scale halved down to 1, or fp16_loss_scale=1, keeps the overflow guard)
    one = torch.ones((), dtype=torch.float32, device=device)       # d loss / d loss, resident (autograd would fill one per step)

    def backward_and_step(loss):
        optimizer.zero_grad()
        scaler.scale(loss).backward(gradient=one)
        if world > 1:        # (SUM of the still-scaled gradients: every rank then sees the same overflow, or none)
            if not brain_encoder.grads_are_reduced:
                allreduce_gradients(params)
            elif clip:       # the temperature's (and the sigmoid loss's bias's) gradient; MSELoss has none
                allreduce_gradients(list(loss_func.parameters()))
        # fp16 only: an activation gradient that overflowed to inf / NaN must not reach Adam — the finiteness check is a
        # host read-back per step of ONE device flag written by one fused launch (fp16 is configs[4]'s dtype; bf16 / fp32
        # never take it), the step is skipped and the scale halved (amp.LossScaler.update, GradScaler's rule).  A skipped
        # step is not a no-op for BatchNorm: its forward has already moved the running statistics and num_batches_tracked
        # (as it would under torch.cuda.amp with nn.BatchNorm1d) — harmless for training, visible in a bit-for-bit replay
        ok = scaler.unscale_(params, check=fp16)
        scaler.update(ok)
        if ok:
            optimizer.step()
    return backward_and_step


def make_guarded_step(brain_encoder, loss_func, params, optimizer, world: int, device):
    """backward_and_step(loss) with the guard on the device (`optimizer`: speech_decoding_amd.optim.GuardedAdam): backward of the
    scaled loss, the same gradient all-reduce as make_backward_and_step, and optimizer.step() — the gradient norm, the overflow
    check, the loss-scale update, clipping and Adam in three launches.  Nothing here reads the device back: the host goes on
    enqueueing the next step.  Under data parallelism the guard runs after the SUM of the still-scaled gradients, so every rank
    reduces the same bits and takes the same decision — no further collective.  A non-finite gradient skips the step in every
    dtype (bf16 / fp32 run at scale 1, not dynamic): torch.nn.utils.clip_grad_norm_ would pass the NaN on to every parameter
    instead; that difference is deliberate.  As in make_backward_and_step, a skipped step has still moved BatchNorm's statistics."""
    clip = isinstance(loss_func, (CLIPLoss, SigmoidLoss))   # a contrastive loss: it has parameters of its own
    one = torch.ones((), dtype=torch.float32, device=device)

    def backward_and_step(loss):
        optimizer.zero_grad()
        optimizer.scale(loss).backward(gradient=one)
        if world > 1:
            if not brain_encoder.grads_are_reduced:
                allreduce_gradients(params)
            elif clip:
                allreduce_gradients(list(loss_func.parameters()))
        optimizer.step()
    return backward_and_step


def guard_mode(args):
    """(guarded, max_grad_norm) from the optional keys max_grad_norm (unset / null: no clipping) and fp16_guard (host: the
    per-step read-back of amp.LossScaler, the default; device: GuardedAdam).  Either one selects the guarded step."""
    where = str(args.get("fp16_guard", "host"))
    if where not in ("host", "device"):
        raise ValueError(f"fp16_guard={where}: expected host or device")
    max_grad_norm = args.get("max_grad_norm", None)
    return where == "device" or max_grad_norm is not None, None if max_grad_norm is None else float(max_grad_norm)


def run(args, train_batches: Optional[Callable] = None, test_batch: Optional[Callable] = None, log=print):
    import torch.distributed as dist
    data_kind = str(args.get("data", "pool"))
    guarded, max_grad_norm = guard_mode(args)          # (an unknown fp16_guard is refused before anything touches the device)
    duplicates = str(args.get("clip_duplicates", "ignore"))
    if duplicates not in ("ignore", "positive", "mask"):
        raise ValueError(f"clip_duplicates={duplicates}: expected ignore, positive or mask")
    if duplicates != "ignore" and str(args.get("loss", "clip")).lower() == "mse":
        raise ValueError(f"clip_duplicates={duplicates} is an option of the contrastive losses; loss=mse has no negatives to correct")
    use_ids = duplicates != "ignore"
    n_neg = int(args.get("clip_negatives", 0))
    if n_neg < 0:
        raise ValueError(f"clip_negatives={n_neg}: expected a number of extra speech negatives per step, 0 for none")
    if n_neg and (train_batches is not None or data_kind != "tracks" or str(args.get("loss", "clip")).lower() != "clip"):
        raise ValueError(f"clip_negatives={n_neg} needs data=tracks (the negatives are windows of the resident speech tracks) and "
                         "loss=clip")
    if train_batches is None and data_kind == "continuous" and args.dataset != "Brennan2018":
        raise ValueError("data=continuous is Brennan2018's input path (one stimulus, every subject): use dataset=Brennan2018")
    if train_batches is None and data_kind == "tracks" and args.dataset != "Gwilliams2022":
        raise ValueError("data=tracks is Gwilliams2022's input path (segments are windows of per-task speech tracks): use "
                         "dataset=Gwilliams2022")
    if train_batches is None and data_kind == "tracks":        # fp32: the feed's own refusal, before anything is built
        D.check_track_dtype("data=tracks", resolve_dtype(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    from speech_decoding_amd.streams import use_training_stream
    caller_stream = torch.cuda.current_stream(device)
    use_training_stream(device)          # the loop's chain on a high-priority stream; the engine's side streams stay normal
    owns_group = world > 1 and not dist.is_initialized()
    if owns_group:
        from speech_decoding_amd.distributed import init_process_group as sda_init_pg
        sda_init_pg(os.environ.get("SDA_DIST_BACKEND", "nccl"))
    if args.get("reproducible", False):
        np.random.seed(0)
        torch.manual_seed(0)
    elif world > 1:
        # SpatialDropout's centre comes from NumPy's global generator (models.py:81) and must be the same on every rank
        from speech_decoding_amd.distributed import seed_numpy_all_ranks
        seed_numpy_all_ranks()

    feed = None          # a resident feed hands out this rank's shard; batches of the pool, or the caller's, are whole and sliced here
    if train_batches is None:
        feed, train_batches, test_batch = build_data(args, data_kind, device, rank, world, with_ids=use_ids, negatives=n_neg)

    def local_shard(batch):
        """(X, Y, subject_idxs, labels, negatives): labels = the batch's speech ids as the loss takes them (checked and uploaded
        once for the loss and the accuracies), or None — clip_duplicates=ignore, or a batch that comes without ids; negatives =
        the bank of extra speech negatives a training batch ends with under clip_negatives, else None."""
        X, Y, subject_idxs = batch[:3]
        neg = batch[-1] if n_neg and isinstance(batch[-1], D.WindowBank) else None
        ids = batch[3] if use_ids and len(batch) - (neg is not None) == 4 else None
        if world > 1 and feed is None:
            lo, hi = shard_range(X.shape[0], rank, world)
            X, Y, subject_idxs = X[lo:hi], Y[lo:hi], subject_idxs[lo:hi]
            ids = None if ids is None else ids[lo:hi]
        return X, Y, subject_idxs, None if ids is None else speech_labels(ids, X.shape[0], device), neg

    brain_encoder = BrainEncoder(args).to(device)
    if feed is not None:
        feed.pack_embeddings(brain_encoder.compute_dtype)      # Y batches arrive as the loss's packed operand
    classifier = Classifier(args)
    loss_kind = str(args.get("loss", "clip")).lower()
    if loss_kind not in ("clip", "sigmoid", "mse"):
        raise ValueError(f"loss={loss_kind}: expected clip, sigmoid or mse")
    clip = loss_kind != "mse"            # a contrastive loss: parameters of its own, the speech-side prefetch, labels
    # (`ignore` is this script's word for "no labels"; the loss itself knows the two ways of using them)
    loss_args = args if use_ids or "clip_duplicates" not in args else type(args)({**args, "clip_duplicates": "positive"})
    loss_func = {"clip": lambda: CLIPLoss(loss_args), "sigmoid": lambda: SigmoidLoss(loss_args), "mse": MSELoss}[loss_kind]().to(device)
    loss_func.train()
    broadcast_parameters(brain_encoder)
    # MSELoss has no parameters of its own: Adam steps the encoder alone
    params = list(brain_encoder.parameters()) + (list(loss_func.parameters()) if clip else [])
    if not guarded:
        optimizer = torch.optim.Adam(params, lr=float(args.lr))
    wandb = None
    if args.get("use_wandb", False) and rank == 0:
        import wandb as _wandb
        wandb = _wandb
        wandb.init(project=args.wandb.project, entity=args.wandb.entity, config=dict(args), save_code=True)
        wandb.run.name = args.wandb.run_name + "_" + str(args.split_mode)

    from speech_decoding_amd.amp import LossScaler
    scaler = LossScaler.for_dtype(brain_encoder.compute_dtype, float(args.get("fp16_loss_scale", 1024.0)),
                                  global_batch=int(args.batch_size), T=D.segment_dims(args).T)     # no-op unless fp16
    if guarded:          # the same starting scale and growth rules, kept and applied on the device (bf16 / fp32: scale 1, fixed)
        from speech_decoding_amd.optim import GuardedAdam
        optimizer = GuardedAdam(params, lr=float(args.lr), max_grad_norm=max_grad_norm, loss_scale=scaler.scale_value,
                                dynamic=scaler.enabled, growth_interval=scaler.growth_interval, max_scale=scaler.max_scale)
        backward_and_step = make_guarded_step(brain_encoder, loss_func, params, optimizer, world, device)
    else:
        backward_and_step = make_backward_and_step(brain_encoder, loss_func, params, optimizer, scaler, world, device)

    history = []
    for epoch in range(int(args.epochs)):
        if epoch == 1:
            # everything allocated so far (model, optimizer state, workspaces) is permanent: keep CPython's full
            # collections from walking it again and again (one costs ~90 ms of host time against an 8 ms step)
            import gc
            gc.collect()
            gc.freeze()
        tr_loss, tr_ranks = [], []
        brain_encoder.train()
        loss = None
        # The speech side of the loss does not depend on the encoder: it is started ONE BATCH AHEAD, like a data loader —
        # batch n + 1's rows are packed (and, under data parallelism, all-gathered: 197 MB per rank at config 3) while batch
        # n's backward runs, five milliseconds of cover instead of the forward's two and a half.  CLIPLoss keeps two packed
        # buffers in rotation for exactly this; only the first batch of an epoch is prefetched at its own start.
        batches = (local_shard(b) for b in train_batches())       # (sharded ONCE per batch: the prefetch is matched by tensor identity)
        ahead = next(batches, None)
        first = True
        while ahead is not None:
            X, Y, subject_idxs, labels, negatives = ahead
            ahead = next(batches, None)
            if first and clip:
                loss_func.prefetch(Y, brain_encoder.compute_dtype)
                first = False
            Z = brain_encoder(X, subject_idxs)
            if negatives is not None:
                loss = loss_func(Y, Z, labels=labels, negatives=negatives)
            else:
                loss = loss_func(Y, Z) if labels is None else loss_func(Y, Z, labels=labels)
            # The reference reads loss.item() and the two accuracies back on the host here, every batch (train.py:194-198):
            # a host<->GPU synchronisation in the middle of the step.  The same numbers are kept on the device and read
            # once per epoch, below: the host keeps enqueueing while the GPU works (8 vs 16 ms per step at batch 256).
            with torch.no_grad():
                ranks = classifier.ranks(Z, Y, labels=labels)    # Classifier.forward's ranks, kept on the device
            tr_loss.append(loss.detach())
            tr_ranks.append(ranks)
            if ahead is not None and clip:
                loss_func.prefetch(ahead[1], brain_encoder.compute_dtype)
            if args.dataset == "Gwilliams2022":
                backward_and_step(loss)
        if args.dataset == "Brennan2018" and loss is not None:          # once per epoch, last batch only
            backward_and_step(loss)
        tr_loss = [float(l) for l in tr_loss]
        tr_top1 = [float((r == 0).float().mean()) for r in tr_ranks]
        tr_top10 = [float((r < 10).float().mean()) for r in tr_ranks]

        brain_encoder.eval()
        te_loss, te_top1, te_top10 = [], [], []
        with torch.no_grad():
            X, Y, subject_idxs, labels, _ = local_shard(test_batch())
            Z = brain_encoder(X, subject_idxs)
            te_loss.append((loss_func(Y, Z) if labels is None else loss_func(Y, Z, labels=labels)).item())
            t1, t10 = classifier(Z, Y, test=True, labels=labels)
            te_top1.append(t1)
            te_top10.append(t10)

        row = {"epoch": epoch, "train_loss": np.mean(tr_loss), "test_loss": np.mean(te_loss),
               "trainTop1acc": np.mean(tr_top1), "trainTop10acc": np.mean(tr_top10),
               "testTop1acc": np.mean(te_top1), "testTop10acc": np.mean(te_top10),
               "lrate": optimizer.param_groups[0]["lr"]}
        if clip:
            row["temp"] = loss_func.temp.item()
        if loss_kind == "sigmoid":
            row["bias"] = loss_func.bias.item()
        if guarded:          # read back here, once per epoch: the last step's unscaled norm and the skips so far
            row["grad_norm"] = optimizer.last_grad_norm
            row["skipped_steps"] = optimizer.skipped_steps
        history.append(row)
        if rank == 0:
            log(f"Ep {epoch}/{args.epochs} | ", f"train l: {row['train_loss']:.3f} | ", f"test l: {row['test_loss']:.3f} | ",
                f"trainTop10acc: {row['trainTop10acc']:.3f} | ", f"testTop10acc: {row['testTop10acc']:.3f} | ",
                f"lr: {row['lrate']:.5f}", *([f"temp: {row['temp']:.3f}"] if clip else []),
                *([f"bias: {row['bias']:.3f}"] if "bias" in row else []))
            if wandb is not None:
                wandb.log(row)
            torch.save(brain_encoder.state_dict(), "model_last.pt")
    if owns_group:                       # a group this function created is also ended here, in order (distributed.shutdown)
        from speech_decoding_amd.distributed import shutdown
        if clip:
            loss_func.drain()
        shutdown()
    # hand the thread back on the stream it came with (everything queued on the training stream is waited for first)
    caller_stream.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.set_stream(caller_stream)
    return history, brain_encoder, loss_func


def main(argv):
    overrides = [a for a in argv if "=" in a and not a.startswith("--")]
    path = next((a.split("=", 1)[1] for a in argv if a.startswith("--config=")), None)
    args = load_config(path, overrides)
    args.setdefault("root_dir", os.getcwd())                       # injected by the reference via open_dict
    args.setdefault("num_subjects", 27 if args.dataset == "Gwilliams2022" else 33)
    t0 = time.time()
    run(args)
    print(f"done in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1:])
