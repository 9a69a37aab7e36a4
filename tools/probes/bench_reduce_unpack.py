"""reduce_unpack_wgrad alone at the step's shapes (diagnostic): the K-split slab sums that follow every weight-gradient GEMM."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # tools/: the harness
from harness import need_gpu, us, window
import torch
from speech_decoding_amd import ops


def main():
    need_gpu()
    for (cout, cin, ks, nseg) in [(320, 320, 3, 25), (640, 320, 3, 12), (320, 320, 3, 51), (1024, 640, 1, 3), (640, 320, 1, 12)]:
        slabs = torch.randn(nseg, ks, cout, cin, device="cuda:0")
        t = us(window(lambda: ops.reduce_unpack_wgrad(slabs, cout, cin, ks), 50, 5))
        mb = slabs.numel() * 4 / 1e6
        print(f"reduce_unpack {cout}x{cin}x{ks} nseg={nseg:3d}: {t:6.1f} us  ({mb:.0f} MB -> {mb / t / 1e3 * 1e3:.0f} GB/s)", flush=True)


if __name__ == "__main__":
    main()
