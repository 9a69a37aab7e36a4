"""MI355X-native `BrainEncoder` / `Classifier` with the reference's constructor and forward signatures
(speech_decoding/models.py:169-248) and state_dict keys, and the reference's submodules
`SpatialAttention`, `SubjectBlock` and `ConvBlock`, which also run on their own.

All of them hold their parameters as the reference does (so `.parameters()`, `.to()`, `.state_dict()`, Adam all work as
with the reference).  `BrainEncoder.forward` runs the whole encoder in libsdamd.so through `engine.EncoderEngine` as ONE
autograd node: it does not call its submodules, so forward hooks registered on them do not fire inside `enc(X, s)`.
Called on their own (`SpatialAttention(X)`, `SubjectBlock(X, subject_idxs)`, `ConvBlock(X)`), the three submodules run
the stage schedules of `blocks.py`, one autograd node per call, and hand back a fresh row-layout buffer as a (B, C_out, T)
view in their compute dtype.  There is no PyTorch fallback for the math.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import lib as L
from . import ops
from .engine import EncoderDims, EncoderEngine
from .layers import block_dilations, subject_indices
from .layout import ch_locations_2d
from . import loss as _loss
from . import blocks as _blocks


def _opt(args, key, default=None):
    if isinstance(args, dict):
        return args.get(key, default)
    return getattr(args, key, default)


def resolve_dtype(args) -> torch.dtype:
    name = os.environ.get("SDA_COMPUTE_DTYPE") or _opt(args, "compute_dtype", "fp32") or "fp32"
    name = str(name).lower()
    if name in ("fp32", "float32", "f32"):
        return torch.float32
    if name in ("bf16", "bfloat16"):
        return torch.bfloat16
    if name in ("fp16", "float16", "half", "f16"):
        return torch.float16
    raise ValueError(f"compute_dtype must be fp32, bf16 or fp16, got {name!r}")


def _dp_group():
    from .distributed import active_group
    return active_group()


def _check_input(X, who: str, channels: int):
    """The (B, C, T) device-tensor contract of the standalone submodules: the reference's shape checks first, then the device
    (there is no CPU path, as elsewhere in the product) and the dtype."""
    if not torch.is_tensor(X) or X.dim() != 3:
        raise ValueError(f"{who}: X must be a (B, C, T) tensor")
    if who == "ConvBlock":
        if X.shape[1] != channels:
            raise RuntimeError(f"ConvBlock: expected input to have {channels} channels, but got {X.shape[1]}")
    else:
        assert X.shape[1] == channels                                             # models.py:78
    if not X.is_cuda:
        raise L.SdaError(f"{who} needs X on the MI355X device (there is no CPU path)")
    if X.dtype not in ops.COMPUTE_DTYPES:
        raise L.SdaError(f"{who}: X of dtype {X.dtype}; the module takes float32, bfloat16 or float16")


class _SpatialAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, X, mask, need_grad, z):
        y, c = _blocks.spatial_attention_forward(module, X, mask, need_grad)
        ctx.module, ctx.bctx = module, c
        ctx.dtype = module.compute_dtype
        B, _, T = X.shape
        return ops.rows_view(y, B, module.z.shape[0], T)

    @staticmethod
    def backward(ctx, dY):
        module = ctx.module
        dYt = _blocks.grad_rows(dY, module.z.shape[0], ctx.dtype)
        dX, dz = _blocks.sa_backward(module, ctx.bctx, dYt, ctx.needs_input_grad[1], ctx.needs_input_grad[4])
        return None, dX, None, None, dz


class _SubjectBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, X, sidx, mask, need_grad, want_subj, z, sb_w, sb_b, subj_w):
        y, c = _blocks.subject_block_forward(module, X, sidx, mask, need_grad, want_subj)
        if c is not None:
            c.params = [sb_w, subj_w]                      # re-packed by the backward
            c.versions = [p._version for p in c.params]
        ctx.module, ctx.bctx = module, c
        ctx.dtype = module.compute_dtype
        B, _, T = X.shape
        return ops.rows_view(y, B, module.D1, T)

    @staticmethod
    def backward(ctx, dY):
        module, n = ctx.module, ctx.needs_input_grad
        if ctx.dtype != module.compute_dtype:
            raise L.SdaError("SubjectBlock: the compute dtype changed between forward and backward")
        dYt = _blocks.grad_rows(dY, module.D1, ctx.dtype)
        g = _blocks.subject_block_backward(module, ctx.bctx, dYt, dict(X=n[1], z=n[6], sb_w=n[7], sb_b=n[8], subj_w=n[9]))
        return (None, g.get("X"), None, None, None, None, g.get("z"), g.get("sb_w"), g.get("sb_b"), g.get("subj_w"))


class _ConvBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, X, need_grad, *params):
        y, c = _blocks.conv_block_forward(module, X, need_grad)
        if c is not None:
            c.params = list(params)
            c.versions = [p._version for p in params]
        ctx.module, ctx.bctx = module, c
        ctx.dtype = module.compute_dtype
        B, _, T = X.shape
        return ops.rows_view(y, B, module.D2, T)

    @staticmethod
    def backward(ctx, dY):
        module, c, n = ctx.module, ctx.bctx, ctx.needs_input_grad
        if ctx.dtype != module.compute_dtype:
            raise L.SdaError("ConvBlock: the compute dtype changed between forward and backward")
        dYt = _blocks.grad_rows(dY, module.D2, ctx.dtype)
        want = dict(zip(_blocks.CB_PARAMS, n[3:]), X=n[1])
        g = _blocks.conv_block_backward(module, c, dYt, want)
        dX = None
        if "X" in g:
            # an RL-view input (the output of another module) gets its gradient as an RL view of the same layout, which that
            # module's backward consumes without a pack; a plain input gets a contiguous tensor of its own dtype
            dX = (ops.rows_view(g["X"], c.B, module.in_channels, c.T) if c.x_rows
                  else ops.unpack_rows(g["X"], c.B, module.in_channels, c.T, c.x_dtype))
        return (None, dX, None, *[g.get(name) for name in _blocks.CB_PARAMS])


class SpatialAttention(nn.Module):
    """models.py:14-86: complex `z` (D1, K²) ~ U[0,1)+iU[0,1), buffers cos/sin (K², C), SpatialDropout in training mode.
    `SpatialAttention(args)(X) -> (B, D1, T)` on HIP kernels (blocks.py), in the compute dtype of `args`."""

    def __init__(self, args):
        super().__init__()
        K = int(args.K)
        loc = ch_locations_2d(args)                                    # (C, 2) in [0.1, 0.9]
        self.z = nn.Parameter(torch.rand(size=(int(args.D1), K * K), dtype=torch.cfloat))
        kk = torch.arange(K).repeat_interleave(K)                       # m = k*K + l
        ll = torch.arange(K).repeat(K)
        phi = 2 * torch.pi * (kk[:, None] * loc[None, :, 0] + ll[:, None] * loc[None, :, 1])
        self.register_buffer("cos", torch.cos(phi))
        self.register_buffer("sin", torch.sin(phi))
        self.loc = loc                                                  # plain attribute, as in the reference
        self.d_drop = float(args.d_drop)
        self._tables_T = None
        self.compute_dtype = resolve_dtype(args)
        self._fixed_centre: Optional[int] = None

    def set_compute_dtype(self, dtype: torch.dtype):
        self.compute_dtype = dtype
        return self

    def set_drop_centre(self, centre: Optional[int]):
        """Testing hook: pin SpatialDropout's centre instead of drawing it from np.random (models.py:81)."""
        self._fixed_centre = centre

    def dropout_mask(self, device) -> Optional[torch.Tensor]:
        """SpatialDropout (models.py:77-86): in training mode one centre per call from NumPy's global RNG (or the pinned one),
        as a row of the device-resident mask table; None (no dropout, no draw) in eval mode."""
        if not self.training:
            return None
        centre = self._fixed_centre if self._fixed_centre is not None else int(np.random.randint(self.loc.shape[0]))
        return self.device_masks(device)[centre]

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        _check_input(X, "SpatialAttention", self.loc.shape[0])
        mask = self.dropout_mask(X.device)
        need_grad = torch.is_grad_enabled() and (X.requires_grad or self.z.requires_grad)
        return _SpatialAttentionFn.apply(self, X, mask, need_grad, self.z)

    def _tables_key(self):
        # rebuilt when the buffers move or are written in place (load_state_dict copies into them)
        return (str(self.cos.device), self.cos.data_ptr(), self.cos._version, self.sin._version)

    def transposed_tables(self):
        key = self._tables_key()
        if self._tables_T is None or self._tables_T[0] != key:
            self._tables_T = (key, self.cos.t().contiguous(), self.sin.t().contiguous())
        return self._tables_T[1], self._tables_T[2]

    def gemm_tables(self):
        """Operand tables of the two contractions of the weight build for the matrix-core path (ops._sa_gemm_tables)."""
        from . import ops
        key = self._tables_key()
        if getattr(self, "_tables_G", None) is None or self._tables_G[0] != key:
            self._tables_G = (key,) + tuple(ops.sa_gemm_tables(self.cos, self.sin))
        return self._tables_G[1], self._tables_G[2]

    def draw_mask(self) -> torch.Tensor:
        """models.py:81-83: one centre per forward from NumPy's global RNG; 0 within d_drop of it."""
        centre = int(np.random.randint(self.loc.shape[0]))
        return self.mask_for(centre)

    def device_masks(self, device) -> torch.Tensor:
        """All C possible dropout masks (row = centre sensor), built once and kept on the device."""
        m = getattr(self, "_masks", None)
        if m is None or m.device != torch.device(device):
            dist = (self.loc[:, None, :] - self.loc[None, :, :]).norm(dim=-1)
            m = self._masks = torch.where(dist < self.d_drop, 0.0, 1.0).to(torch.float32).to(device)
        return m

    def mask_for(self, centre: int) -> torch.Tensor:
        dist = (self.loc - self.loc[centre]).norm(dim=-1)
        return torch.where(dist < self.d_drop, 0.0, 1.0).to(torch.float32)


class SubjectLayers(nn.Module):
    """The reference's ModuleList of S bias-free 1x1 convs (models.py:98-109) stored as ONE (S, D1, D1, 1)
    parameter so a kernel can select the matrix by subject index; state_dict keys stay `{s}.weight`."""

    def __init__(self, num_subjects: int, D1: int):
        super().__init__()
        ws = [nn.Conv1d(D1, D1, kernel_size=1, bias=False).weight.detach() for _ in range(num_subjects)]
        self.weight = nn.Parameter(torch.stack(ws))                     # same RNG draws as S Conv1d inits
        self.num_subjects = num_subjects

    def __len__(self):
        return self.num_subjects

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for s in range(self.num_subjects):
            w = self.weight[s]
            destination[f"{prefix}{s}.weight"] = w if keep_vars else w.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for s in range(self.num_subjects):
            key = f"{prefix}{s}.weight"
            if key in state_dict:
                with torch.no_grad():
                    self.weight[s].copy_(state_dict[key])
            elif strict:
                missing_keys.append(key)
        if strict:
            for key in state_dict:
                if key.startswith(prefix) and key[len(prefix):].split(".")[0].isdigit():
                    if int(key[len(prefix):].split(".")[0]) >= self.num_subjects:
                        unexpected_keys.append(key)


class SubjectBlock(nn.Module):
    """models.py:89-117: SpatialAttention, a shared 1x1 conv with bias, a per-subject 1x1 conv without bias.
    `SubjectBlock(args)(X, subject_idxs) -> (B, D1, T)` on HIP kernels (blocks.py), in the compute dtype of `args`."""

    def __init__(self, args):
        super().__init__()
        D1 = int(args.D1)
        self.num_subjects, self.D1, self.K = int(args.num_subjects), D1, int(args.K)
        self.spatial_attention = SpatialAttention(args)
        self.conv = nn.Conv1d(D1, D1, kernel_size=1, stride=1)
        self.subject_layer = SubjectLayers(int(args.num_subjects), D1)
        self.compute_dtype = self.spatial_attention.compute_dtype

    def set_compute_dtype(self, dtype: torch.dtype):
        self.compute_dtype = dtype
        self.spatial_attention.set_compute_dtype(dtype)
        return self

    def forward(self, X: torch.Tensor, subject_idxs) -> torch.Tensor:
        sa = self.spatial_attention
        _check_input(X, "SubjectBlock", sa.loc.shape[0])
        sidx = subject_indices(subject_idxs, X.shape[0], self.num_subjects)
        mask = sa.dropout_mask(X.device)                     # the one draw of this call, through its SpatialAttention
        params = [sa.z, self.conv.weight, self.conv.bias, self.subject_layer.weight]
        grad_mode = torch.is_grad_enabled()
        need_grad = grad_mode and (X.requires_grad or any(p.requires_grad for p in params))
        want_subj = need_grad and self.subject_layer.weight.requires_grad
        return _SubjectBlockFn.apply(self, X, sidx, mask, need_grad, want_subj, *params)


class ConvBlock(nn.Module):
    """models.py:120-166.  `ConvBlock(k, D1, D2)(X) -> (B, D2, T)` on HIP kernels (blocks.py).  With no `args` to read, its
    compute dtype is resolve_dtype({}) (fp32 unless SDA_COMPUTE_DTYPE is set); `set_compute_dtype` changes it, and a
    BrainEncoder sets its own on its blocks."""

    def __init__(self, k: int, D1: int, D2: int):
        super().__init__()
        cin = D1 if k == 0 else D2
        self.k, self.D2, self.in_channels = k, D2, cin
        self.compute_dtype = resolve_dtype({})
        d0, d1, d2 = block_dilations(k)
        self.conv0 = nn.Conv1d(cin, D2, kernel_size=3, padding="same", dilation=d0)
        self.batchnorm0 = nn.BatchNorm1d(D2)
        self.conv1 = nn.Conv1d(D2, D2, kernel_size=3, padding="same", dilation=d1)
        self.batchnorm1 = nn.BatchNorm1d(D2)
        self.conv2 = nn.Conv1d(D2, 2 * D2, kernel_size=3, padding="same", dilation=d2)

    def set_compute_dtype(self, dtype: torch.dtype):
        self.compute_dtype = dtype
        return self

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        _check_input(X, "ConvBlock", self.in_channels)
        params = _blocks.cb_params(self)
        need_grad = torch.is_grad_enabled() and (X.requires_grad or any(p.requires_grad for p in params))
        return _ConvBlockFn.apply(self, X, need_grad, *params)


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module: "BrainEncoder", X, subject_idxs, mask, need_grad, x_grad, param_grads, *params):
        P = module._param_dict(params)
        ectx = module.engine.forward(P, X, subject_idxs, training=module.training, mask=mask, need_grad=need_grad,
                                     need_dx=x_grad, param_grads=param_grads)
        ctx.module, ctx.ectx, ctx.P = module, ectx, P
        ctx.nparams = len(params)
        B, _, T = X.shape
        return ops.rows_view(ectx.bufs["Z"], B, module.F, T)

    @staticmethod
    def backward(ctx, dZ):
        module, ectx = ctx.module, ctx.ectx
        P = ctx.P
        dZt = _loss.as_rows(dZ, ectx.B, module.F, ectx.T, module.engine.dtype, "dZ")
        g = module.engine.backward(P, ectx, dZt)
        need = ctx.needs_input_grad[7:]
        out = [g.get(name) if n else None for name, n in zip(module._param_names, need)]
        dX = g.get("X") if ctx.needs_input_grad[1] else None
        return (None, dX, None, None, None, None, None, *out)


class BrainEncoder(nn.Module):
    """Drop-in for models.py:169-196: `BrainEncoder(args)(X, subject_idxs) -> (B, F, T)`.

    The returned tensor is a zero-copy (B, F, T) *view* of the channels-last buffer the kernels wrote
    (strides (Tp*Fp, 1, Fp)); `CLIPLoss` / `Classifier` from this package consume it without a copy."""

    def __init__(self, args):
        super().__init__()
        self.num_subjects = int(args.num_subjects)
        self.D1, self.D2, self.K = int(args.D1), int(args.D2), int(args.K)
        self.F = int(args.F) if not args.preprocs["last4layers"] else 1024          # models.py:176
        self.dataset_name = args.dataset
        self.compute_dtype = resolve_dtype(args)

        self.subject_block = SubjectBlock(args)
        self.conv_blocks = nn.Sequential()
        for k in range(5):
            self.conv_blocks.add_module(f"conv{k}", ConvBlock(k, self.D1, self.D2))
        self.conv_final1 = nn.Conv1d(self.D2, 2 * self.D2, kernel_size=1)
        self.conv_final2 = nn.Conv1d(2 * self.D2, self.F, kernel_size=1)

        self.sync_batchnorm = True          # under torch.distributed: BN statistics over the global batch
        self._engine: Optional[EncoderEngine] = None
        self._fixed_centre: Optional[int] = None
        self.drop_centre_sync = "seed"        # under data parallelism: "seed" (identical np.random on all ranks, checked) | "broadcast"
        self._centre_draws = 0
        self._param_names = self._build_names()
        self._set_children_dtype()

    def _set_children_dtype(self):
        """The submodules, when called on their own, compute in the encoder's dtype."""
        self.subject_block.set_compute_dtype(self.compute_dtype)
        for blk in self.conv_blocks:
            blk.set_compute_dtype(self.compute_dtype)

    # ---- parameter plumbing -------------------------------------------------------------
    def _build_names(self) -> List[str]:
        names = ["z", "sb_w", "sb_b", "subj_w"]
        for k in range(5):
            names += [f"b{k}.c0w", f"b{k}.c0b", f"b{k}.bn0w", f"b{k}.bn0b", f"b{k}.c1w", f"b{k}.c1b",
                      f"b{k}.bn1w", f"b{k}.bn1b", f"b{k}.c2w", f"b{k}.c2b"]
        return names + ["f1w", "f1b", "f2w", "f2b"]

    def _ordered_params(self) -> List[torch.Tensor]:
        sb = self.subject_block
        ps = [sb.spatial_attention.z, sb.conv.weight, sb.conv.bias, sb.subject_layer.weight]
        for k in range(5):
            blk = getattr(self.conv_blocks, f"conv{k}")
            ps += [blk.conv0.weight, blk.conv0.bias, blk.batchnorm0.weight, blk.batchnorm0.bias,
                   blk.conv1.weight, blk.conv1.bias, blk.batchnorm1.weight, blk.batchnorm1.bias,
                   blk.conv2.weight, blk.conv2.bias]
        return ps + [self.conv_final1.weight, self.conv_final1.bias, self.conv_final2.weight, self.conv_final2.bias]

    def _param_dict(self, params) -> Dict[str, torch.Tensor]:
        P = {n: p.detach() for n, p in zip(self._param_names, params)}
        sa = self.subject_block.spatial_attention
        P["cos"], P["sin"] = sa.cos, sa.sin
        P["cosT"], P["sinT"] = sa.transposed_tables()
        P["sa_tab_f"], P["sa_tab_b"] = sa.gemm_tables() if sa.cos.is_cuda else (None, None)
        for k in range(5):
            blk = getattr(self.conv_blocks, f"conv{k}")
            for j, bn in ((0, blk.batchnorm0), (1, blk.batchnorm1)):
                P[f"b{k}.bn{j}rm"], P[f"b{k}.bn{j}rv"] = bn.running_mean, bn.running_var
                P[f"b{k}.bn{j}nbt"] = bn.num_batches_tracked        # counted by the statistics kernel itself (training mode)
        return P

    @property
    def engine(self) -> EncoderEngine:
        if self._engine is None or self._engine.dtype != self.compute_dtype:
            C = self.subject_block.spatial_attention.cos.shape[1]
            self._engine = EncoderEngine(EncoderDims(C, self.num_subjects, self.D1, self.D2, self.F, self.K),
                                         self.compute_dtype, group=_dp_group() if self.sync_batchnorm else None)
        return self._engine

    @property
    def grads_are_reduced(self) -> bool:
        """True when backward already SUM-all-reduced this module's gradients across ranks (data parallel,
        overlapped with backward); callers then all-reduce only what lives outside the encoder (CLIPLoss.temp)."""
        e = self.engine
        return e.group is not None and e.overlap_grad_allreduce

    def set_compute_dtype(self, dtype: torch.dtype):
        self.compute_dtype = dtype
        self._set_children_dtype()
        return self

    def set_drop_centre(self, centre: Optional[int]):
        """Testing hook: pin SpatialDropout's centre instead of drawing it from np.random (models.py:81)."""
        self._fixed_centre = centre

    # ---- forward ------------------------------------------------------------------------
    def forward(self, X: torch.Tensor, subject_idxs) -> torch.Tensor:
        sa = self.subject_block.spatial_attention
        assert X.shape[1] == sa.loc.shape[0]                                      # models.py:78
        if torch.is_grad_enabled() and X.requires_grad and X.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise L.SdaError(f"BrainEncoder: X of dtype {X.dtype} requires a gradient; its gradient is computed for float32, "
                             "bfloat16 and float16 inputs only")
        if not X.is_cuda:
            raise L.SdaError("BrainEncoder needs X on the MI355X device (there is no CPU path)")
        mask = None
        if self.training:
            if self._fixed_centre is not None:
                centre = self._fixed_centre
            else:
                centre = int(np.random.randint(sa.loc.shape[0]))            # models.py:81, NumPy global RNG
            mask = sa.device_masks(X.device)[centre]            # (C, C) table resident on the device: no upload
            group = _dp_group()
            if group is not None and self._fixed_centre is None:
                # "same drop centre for all samples in batch" (models.py:69) — the batch is global, so every rank must use
                # the same centre.  NumPy's global generator is seeded identically on all ranks
                # (distributed.seed_numpy_all_ranks; train.py / bench.py do it) and nothing else draws from it, so every
                # rank draws the same centre by itself: no collective in front of the forward.  That lockstep is CHECKED —
                # on the first data-parallel forward and every 256th after it (one small all-gather + a host read-back) —
                # and a divergence is an error, not a silent semantic change.  drop_centre_sync = "broadcast" restores the
                # per-step broadcast of rank 0's mask (a latency-bound collective on the critical path) for callers that
                # draw from np.random elsewhere.
                import torch.distributed as dist
                if self.drop_centre_sync == "broadcast":
                    mask = mask.clone()         # the cached table must not be overwritten by the broadcast
                    dist.broadcast(mask, src=0, group=group)
                else:
                    if self._centre_draws % 256 == 0:
                        mine = torch.tensor([centre], dtype=torch.int32, device=X.device)
                        allc = torch.empty(dist.get_world_size(group), dtype=torch.int32, device=X.device)
                        dist.all_gather_into_tensor(allc, mine, group=group)
                        if len(set(allc.tolist())) != 1:
                            raise L.SdaError(f"SpatialDropout centres differ across ranks ({allc.tolist()}): NumPy's global generator "
                                             "is out of step — call speech_decoding_amd.distributed.seed_numpy_all_ranks() after "
                                             "init_process_group and draw from np.random on all ranks alike, or set "
                                             "brain_encoder.drop_centre_sync = 'broadcast'")
                    self._centre_draws += 1
        params = self._ordered_params()
        grad_mode = torch.is_grad_enabled()                  # (grad mode is off inside Function.forward)
        param_grads = grad_mode and any(p.requires_grad for p in params)
        x_grad = grad_mode and X.requires_grad
        # X requiring a gradient with every parameter frozen (saliency maps, a trained encoder behind a learnable front end):
        # the backward runs the data-gradient chain only
        return _EncoderFn.apply(self, X, subject_idxs, mask, param_grads or x_grad, x_grad, param_grads, *params)


class Classifier(nn.Module):
    """Drop-in for models.py:199-248: top-1 / top-10 retrieval accuracy of speech rows against brain
    columns.  The B² Python loop is one similarity GEMM + a rank kernel; results equal the reference's
    ranking because logits are a positive rescaling of the cosine similarities."""

    def __init__(self, args=None):
        super().__init__()
        self.factor = 1
        self.global_candidates = True       # under torch.distributed: rank against the global batch

    @torch.no_grad()
    def ranks(self, Z: torch.Tensor, Y: torch.Tensor, labels=None) -> torch.Tensor:
        """Rank of every speech row's own brain column (0 = top-1) as a DEVICE tensor: what forward() reduces to the two
        accuracies, without the host read-back (a training loop can collect these and read them once per epoch).
        `labels`: the local samples' speech ids (as CLIPLoss.forward takes them); a brain column that heard the row's own
        speech segment then never counts as a wrong answer."""
        if Z.size(0) < 10:
            raise RuntimeError("selected index k out of range")      # torch.topk(…, 10) on fewer than 10 columns
        return _loss.retrieval_ranks(Y, Z, self.global_candidates, labels=labels)

    @torch.no_grad()
    def decode(self, Z: torch.Tensor, bank, k: int = 10, labels=None):
        """Decode brain segments against a speech bank: the QUERIES are the brain embeddings Z (N, F, T), the CANDIDATES the
        speech segments of `bank` (a retrieval.SpeechBank, or a retrieval.WindowBank of windows cut from continuous tracks); returns retrieval.retrieve(Z, bank, k, labels) — for each brain
        segment the k best speech candidates and, with `labels`, the rank of the one it heard.  forward() looks the other
        way (for each speech row, the brain columns of the batch); retrieve() serves either direction, it does not care which
        side is which."""
        from .retrieval import retrieve
        return retrieve(Z, bank, k=k, labels=labels)

    @torch.no_grad()
    def decode_classes(self, Z: torch.Tensor, bank, classes, **kw):
        """Word-level decoding of brain segments: the QUERIES are the brain embeddings Z (N, F, T), the CANDIDATES the speech
        segments of `bank` (a retrieval.SpeechBank or retrieval.WindowBank), `classes` says which word each candidate is an instance of (a retrieval.ClassIndex or the M class
        ids); returns retrieval.retrieve_classes(Z, bank, classes, **kw) — for each brain segment (or, with groups=, each group
        of repetitions) the k most probable words and, with labels=, the rank of the one it heard."""
        from .retrieval import retrieve_classes
        return retrieve_classes(Z, bank, classes, **kw)

    @torch.no_grad()
    def forward(self, Z: torch.Tensor, Y: torch.Tensor, test: bool = False, labels=None):
        cnt = self.ranks(Z, Y, labels=labels).cpu().numpy()
        return float((cnt == 0).mean()), np.mean(cnt < 10)
