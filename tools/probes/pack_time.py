"""pack_rows at the step's two shapes, fp32 and bf16 sources (diagnostic)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # tools/: the harness
from harness import need_gpu, us, window
import torch
from speech_decoding_amd import ops


def main():
    need_gpu()
    dev = "cuda:0"
    for name, B, C, T, Cp in [("X 208 -> 256", 256, 208, 360, 256), ("Y 1024", 256, 1024, 360, 1024)]:
        x32 = torch.randn(B, C, T, device=dev)
        for x in (x32, x32.bfloat16()):
            for dt in (torch.bfloat16, torch.float32):
                buf = ops.new_rows(B, T, Cp, dt, dev)
                t = us(window(lambda: ops.pack_rows(x, buf), 20, 3))
                mb = (x.numel() * x.element_size() + B * T * Cp * buf.element_size()) / 1e6
                print(f"{name:14s} {str(x.dtype)[6:]:8s} -> {str(dt)[6:]:9s} {t:7.1f} us  {mb:6.0f} MB  {mb / t:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
