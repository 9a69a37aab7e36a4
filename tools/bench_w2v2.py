"""Throughput of the frozen wav2vec 2.0 embedder at a published checkpoint's dimensions (diagnostic; random weights).

    python tools/bench_w2v2.py [seconds_of_audio] [dtype] [variant ...] [--out FILE] [--no-hf]

variant: `xlsr` (default: facebook/wav2vec2-large-xlsr-53, layer-norm feature encoder, stable layer norm), `base`
(wav2vec2-base / -base-960h: group norm, post-LN, 768 x 12 layers, no conv bias) or `large-960h` (wav2vec2-large / -large-960h:
group norm, post-LN, 1024 x 24 layers, no conv bias); several may be given and are then measured in one run.  Per variant:
`embed()` of the whole waveform (ten chunks, as the reference calls it) in ms per call; for the group-norm variants also
`conv_features()` of the whole waveform and the two layer-0 normalisation launches alone (`sda_w2v_conv0_stats`,
`sda_w2v_conv0_groupnorm`) for one chunk and for the whole file, device events after warm-up, with the bytes they must move
(statistics: the waveform read once; normalising: the waveform read once and the row-layout output written once) against
the 8 TB/s HBM rate (MI355X data sheet).  When `transformers` is importable, the same model in the same dtype on the same GPU
through the reference's chunked last-four mean, alternating call by call with `embed()`.  Every line is one JSON object,
printed and appended to --out (kept as profiles/w2v2_variants_bench.json)."""
import argparse

import torch

import harness
from speech_decoding_amd import ops
from speech_decoding_amd.wav2vec2 import Wav2Vec2Config, Wav2Vec2Embedder, chunk_bounds

HBM_PEAK_TBS = 8.0
VARIANTS = {
    "xlsr": dict(),
    "base": dict(conv_bias=False, hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12,
                 feat_extract_norm="group", do_stable_layer_norm=False),
    "large-960h": dict(conv_bias=False, feat_extract_norm="group", do_stable_layer_norm=False),
}


def random_state_dict(cfg, g):
    sd = {}
    def lin(n, o, i): sd[n + ".weight"] = torch.randn(o, i, generator=g) * (0.7 / i ** 0.5); sd[n + ".bias"] = torch.randn(o, generator=g) * 0.1
    def ln(n, c): sd[n + ".weight"] = 1 + 0.1 * torch.randn(c, generator=g); sd[n + ".bias"] = 0.1 * torch.randn(c, generator=g)
    cin, H, F = 1, cfg.hidden_size, cfg.intermediate_size
    for i, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
        p = f"feature_extractor.conv_layers.{i}."
        sd[p + "conv.weight"] = torch.randn(c, cin, k, generator=g) * (0.7 / (cin * k) ** 0.5)
        if cfg.conv_bias:
            sd[p + "conv.bias"] = torch.randn(c, generator=g) * 0.1
        if cfg.feat_extract_norm == "layer" or i == 0:
            ln(p + "layer_norm", c)
        cin = c
    ln("feature_projection.layer_norm", cin); lin("feature_projection.projection", H, cin)
    K, G = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
    sd["encoder.pos_conv_embed.conv.weight_g"] = 0.5 + torch.rand(1, 1, K, generator=g)
    sd["encoder.pos_conv_embed.conv.weight_v"] = torch.randn(H, H // G, K, generator=g) * 0.05
    sd["encoder.pos_conv_embed.conv.bias"] = torch.randn(H, generator=g) * 0.1
    ln("encoder.layer_norm", H)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"): lin(p + "attention." + n, H, H)
        ln(p + "layer_norm", H); ln(p + "final_layer_norm", H)
        lin(p + "feed_forward.intermediate_dense", F, H); lin(p + "feed_forward.output_dense", H, F)
    return sd


def gemm_flop_per_frame(cfg):
    H, F, C = cfg.hidden_size, cfg.intermediate_size, cfg.conv_dim[0]
    conv = sum(k * m for k, m in zip(cfg.conv_kernel[1:], (16, 8, 4, 2, 1, 1)))       # frames of layer i per output frame
    return (2 * (4 * H * H + 2 * H * F) * cfg.num_hidden_layers + 2 * cfg.num_conv_pos_embeddings * (H // cfg.num_conv_pos_embedding_groups) * H
            + 2 * C * H + 2 * C * C * conv)


def mean_min_max(ms, digits):
    s = harness.summarize(ms)
    return {"ms": round(s.mean, digits), "min_ms": round(s.min, digits), "max_ms": round(s.max, digits)}


def timed(fn, iters, warmup):
    """every call between its own pair of events"""
    return mean_min_max(harness.alternating((fn,), iters, warmup)[0], 4)


def timed_pair(fa, fb, iters, warmup):
    """fa and fb alternating call by call, wall clock around a device synchronisation: (ms of fa, ms of fb)"""
    for _ in range(warmup):
        fa(); fb()
    ms = ([], [])
    for _ in range(iters):
        for k, fn in enumerate((fa, fb)):
            ms[k].append(harness.host_clock(fn, 1, 0)[1])
    return tuple(mean_min_max(m, 3) for m in ms)


def hf_model(cfg, sd, dtype):
    import transformers as tr
    hc = tr.Wav2Vec2Config(conv_dim=list(cfg.conv_dim), conv_kernel=list(cfg.conv_kernel), conv_stride=list(cfg.conv_stride),
                           conv_bias=cfg.conv_bias, hidden_size=cfg.hidden_size, num_attention_heads=cfg.num_attention_heads,
                           intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
                           num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
                           num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, layer_norm_eps=cfg.layer_norm_eps,
                           feat_extract_norm=cfg.feat_extract_norm, do_stable_layer_norm=cfg.do_stable_layer_norm,
                           num_feat_extract_layers=len(cfg.conv_dim), apply_spec_augment=False)
    model = tr.Wav2Vec2Model(hc).eval()
    own = model.state_dict()
    g, v = "encoder.pos_conv_embed.conv.weight_g", "encoder.pos_conv_embed.conv.weight_v"
    sd = dict(sd)
    if g not in own:                                   # parametrize-era key names
        sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = sd.pop(g)
        sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = sd.pop(v)
    missing = model.load_state_dict(sd, strict=False)
    assert set(missing.missing_keys) <= {"masked_spec_embed"} and not missing.unexpected_keys, missing
    return model.to("cuda:0").to(dtype), tr.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("seconds", nargs="?", type=float, default=60.0)
    ap.add_argument("dtype", nargs="?", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("variants", nargs="*", default=["xlsr"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-hf", action="store_true")
    a = ap.parse_args()
    for v in a.variants:
        if v not in VARIANTS:
            raise SystemExit(f"variant {v!r}: one of {sorted(VARIANTS)}")
    secs = a.seconds
    dtype = dict(bf16=torch.bfloat16, fp16=torch.float16, fp32=torch.float32)[a.dtype]
    es = 4 if dtype == torch.float32 else 2

    harness.need_gpu()

    def emit(rec):
        harness.emit(rec, a.out, append=True)

    for name in a.variants:
        cfg = Wav2Vec2Config(**VARIANTS[name])
        g = torch.Generator().manual_seed(0)
        sd = random_state_dict(cfg, g)
        emb = Wav2Vec2Embedder(sd, cfg, dtype=dtype)
        wave = torch.randn(1, int(secs * 16000), generator=g).cuda()
        base = {"bench": "w2v2", "variant": name, "dtype": a.dtype, "seconds": secs, "samples": wave.shape[1],
                "feat_extract_norm": cfg.feat_extract_norm, "do_stable_layer_norm": cfg.do_stable_layer_norm,
                "hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_hidden_layers}
        n = 3
        dt = harness.host_clock(lambda: emb.embed(wave), n, 2)[1] * 1e-3
        out = emb.embed(wave)
        frames = out.shape[1]
        flop = frames * gemm_flop_per_frame(cfg)
        print(f"{name}: {secs:.0f} s of audio, {frames} frames, {str(dtype)[6:]}: {dt * 1e3:.1f} ms per call = {secs / dt:.0f} x real time, "
              f"{frames / dt:.0f} frames/s, ~{flop / dt / 1e12:.0f} TFLOP/s (GEMM FLOPs, attention excluded)")
        emit(dict(base, line="embed", what="embed(): ten chunks, four in flight, HIP graphs", ms=round(dt * 1e3, 3), iters=n, frames=frames,
                  x_real_time=round(secs / dt, 1), gemm_tflops=round(flop / dt / 1e12, 1)))
        if cfg.feat_extract_norm == "group":
            emit(dict(base, line="conv_features", what="conv_features(): feature encoder alone on the whole waveform, allocation included",
                      **timed(lambda: emb.conv_features(wave), 5, 2)))
            C, K, S, P = cfg.conv_dim[0], cfg.conv_kernel[0], cfg.conv_stride[0], emb.P
            for label, w1 in (("one chunk", wave[0, :chunk_bounds(wave.shape[1])[0][1]]), ("whole file", wave[0])):
                T0 = (w1.numel() - K) // S + 1
                scratch = torch.empty(ops.w2v_conv0_stats_floats(T0, C), dtype=torch.float32, device="cuda:0")
                y = ops.new_rows(1, T0, emb.Cp, dtype, "cuda:0")
                stats = ops.w2v_conv0_stats(w1, P["c0.w"], P["c0.b"], scratch, T0, C, K, S)
                t_s = timed(lambda: ops.w2v_conv0_stats(w1, P["c0.w"], P["c0.b"], scratch, T0, C, K, S), 20, 5)
                t_n = timed(lambda: ops.w2v_conv0_groupnorm(w1, P["c0.w"], P["c0.b"], P["c0.g"], P["c0.be"], stats, y, T0, C, K, S), 20, 5)
                b_s = 4.0 * w1.numel() + 4.0 * scratch.numel()
                b_n = 4.0 * w1.numel() + float(es) * T0 * emb.Cp
                for kern, t, b in (("sda_w2v_conv0_stats (two launches)", t_s, b_s), ("sda_w2v_conv0_groupnorm", t_n, b_n)):
                    emit(dict(base, line="groupnorm_kernel", kernel=kern, span=label, frames0=T0, channels=C, **t, bytes=int(b),
                              tb_per_s=round(b / (t["ms"] * 1e-3) / 1e12, 3), share_of_hbm_peak=round(b / (t["ms"] * 1e-3) / 1e12 / HBM_PEAK_TBS, 4),
                              conv_gflop=round(2.0 * T0 * C * K / 1e9, 2)))
        if a.no_hf:
            continue
        try:
            model, version = hf_model(cfg, sd, dtype)
        except ImportError:
            emit(dict(base, line="transformers", available=False, what="`transformers` is not importable here: not measured"))
            continue
        except Exception as e:                                                  # noqa: BLE001  (a diagnostic: say why, go on)
            emit(dict(base, line="transformers", available=True, error=repr(e)[:300]))
            continue

        def hf_embed():
            with torch.no_grad():
                outs = []
                for lo, hi in chunk_bounds(wave.shape[1]):
                    hs = model(input_values=wave[:, lo:hi].to(dtype), output_hidden_states=True).hidden_states
                    outs.append(torch.stack(hs[-4:]).mean(0)[0])
                return torch.vstack(outs).t()
        try:
            ref = hf_embed().float()
            ours, theirs = timed_pair(lambda: emb.embed(wave), hf_embed, 3, 1)
            rel = float((out.double() - ref.double()).norm() / ref.double().norm())
            emit(dict(base, line="transformers", available=True, version=version, what="embed() | HF Wav2Vec2Model, same weights, dtype and "
                      "GPU, ten chunks one after the other, last-four mean; alternating call by call, wall clock", **ours, torch=theirs,
                      hf_ms_over_ms=round(theirs["ms"] / ours["ms"], 2), rel_l2_vs_hf=rel))
        except Exception as e:                                                  # noqa: BLE001
            emit(dict(base, line="transformers", available=True, version=version, error=repr(e)[:300]))
        del model
        emb.release_workspace()


if __name__ == "__main__":
    main()
