"""What a test file needs to stand up a model on the oracle's parameters, written once: the argument object, the toy problem,
the encoder and loss builders, and gradients by parameter name.  A plain module: no fixtures."""
import numpy as np
import torch

from oracle import brain_oracle as O
from speech_decoding_amd.config import Config      # noqa: F401  (the dict with attribute access every model takes)

TOY = dict(C=20, S=3, D1=32, D2=48, F=64, K=4, T=70)


def toy_problem(d, B, loc_seed=1, param_seed=2, batch_seed=3):
    """(loc, P, X, Y, subj) of the oracle at dims `d`, batch B; the default seeds are the data-parallel tests'."""
    loc = O.synthetic_positions(d["C"], seed=loc_seed)
    P = O.seeded_params(d["C"], d["S"], d["D1"], d["D2"], d["F"], d["K"], seed=param_seed, loc=loc)
    X, Y, subj = O.synthetic_batch(B, d["C"], d["T"], d["F"], d["S"], seed=batch_seed)
    return loc, P, X, Y, subj


def encoder_args(d, loc, dtype="fp32", last4layers=False, **extra):
    """The Config a BrainEncoder, SubjectBlock or SpatialAttention takes for dims `d` (S, D1, D2, K and, for the encoder, F) and
    sensor positions `loc`.  With positions given the models never read root_dir; `extra` adds or overrides fields (an F of the
    call site's own, reduction / init_temperature where the same Config also feeds CLIPLoss)."""
    fields = dict(num_subjects=d["S"], D1=d["D1"], D2=d["D2"], K=d["K"], dataset="Gwilliams2022", d_drop=0.1,
                  root_dir="/nonexistent", preprocs={"last4layers": last4layers}, sensor_positions=np.asarray(loc),
                  compute_dtype=dtype)
    if "F" in d:
        fields["F"] = d["F"]
    fields.update(extra)
    return Config(fields)


def build_encoder(P, args_or_d, dev, *, training=True, strict=True):
    """BrainEncoder on the state P: nothing missing, nothing unexpected; on `dev`, in train or eval mode.  Dims instead of a
    Config: fp32, sensor positions of seed 1 (toy_problem's default)."""
    from speech_decoding.models import BrainEncoder
    args = args_or_d if isinstance(args_or_d, Config) else encoder_args(args_or_d, O.synthetic_positions(args_or_d["C"], seed=1))
    enc = BrainEncoder(args)
    missing, unexpected = enc.load_state_dict(P, strict=strict)
    assert not missing and not unexpected, (missing, unexpected)
    return enc.to(dev).train(training)


def clip_loss(temp, dev, reduction="mean"):
    from speech_decoding.utils.loss import CLIPLoss
    return CLIPLoss(Config(reduction=reduction, init_temperature=temp)).to(dev)


def grads_of(module, *extra_params):
    """{parameter name: gradient as a real-valued CPU clone} (view_as_real for the complex z); extra_params: (name, parameter)
    pairs from outside the module, such as ("temp", lossf.temp)."""
    named = list(module.named_parameters()) + list(extra_params)
    return {n: (torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad).detach().cpu().clone() for n, p in named}


def null_bias_grad(key):
    """conv0 / conv1 biases of a ConvBlock feed a training-mode BatchNorm: their gradient is zero up to rounding noise."""
    return key.startswith("conv_blocks.") and key.endswith((".conv0.bias", ".conv1.bias"))


def grads_by_state_key(enc):
    """{state key of the reference: gradient}: the per-subject weight split like the reference's ModuleList."""
    out = {}
    for n, p in enc.named_parameters():
        if n == "subject_block.subject_layer.weight":
            for s in range(p.shape[0]):
                out[f"subject_block.subject_layer.{s}.weight"] = None if p.grad is None else p.grad[s]
        else:
            out[n] = p.grad
    return out
