"""Throughput of the GPU collate at the bench's batch (diagnostic): sda_collate_rows on a resident (B, C, T) batch
(Gwilliams2022Collator, gwilliams2022.py:640-661) and sda_collate_windows on resident recordings (ResidentSegments: the
window gather of gwilliams2022.py:129-142 fused with it) — rows/s, GB/s of algorithmic traffic (one read + one write of the
batch) and the share of a 7 ms training step one batch costs."""
import numpy as np
import torch

from harness import need_gpu, us, window
from speech_decoding_amd.collate import ResidentSegments, robust_scale_clamp


def main():
    need_gpu()
    dev = "cuda:0"
    for (B, C, T, nb, name) in [(256, 208, 360, 60, "config 2 (208 ch x 360, batch 256)"), (512, 60, 360, 60, "config 4 per rank (60 ch, batch 512)"),
                                (512, 306, 1000, 100, "config 5 per rank (306 ch x 1000, batch 512)")]:
        X = torch.randn(B, C, T, device=dev) * 3 + 0.5
        t = us(window(lambda: robust_scale_clamp(X, nb, 20.0, True), 20, 3))
        rows, byt = B * C, 2.0 * B * C * T * 4
        print(f"collate_rows    {name:46s} {t:8.1f} us  {rows / t:8.2f} M rows/s  {byt / t / 1e3:7.1f} GB/s", flush=True)
        sessions = [torch.randn(C, 60000, device=dev) for _ in range(8)]
        rs = ResidentSegments(sessions, T, nb, 20.0, True)
        rng = np.random.RandomState(0)
        sidx, on = rng.randint(0, 8, B), rng.randint(0, 60000 - T, B)
        t2 = us(window(lambda: rs.batch(sidx, on), 20, 3))
        print(f"collate_windows {name:46s} {t2:8.1f} us  {rows / t2:8.2f} M rows/s  {byt / t2 / 1e3:7.1f} GB/s  (incl. the host's index upload)", flush=True)


if __name__ == "__main__":
    main()
