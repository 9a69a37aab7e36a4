"""Where the HOST's time goes in a data-parallel step (diagnostic): the headline step with the data-parallel path on at world
size 1 (SDA_DP_SINGLE_RANK=1, emulate_world(N)), 30 steps under cProfile.
    python tools/probes/host_profile_dp.py [N=2]"""
import cProfile, os, pstats, socket, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # tools/: the harness
import harness
import torch


def main():
    harness.need_gpu()
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if N > 1:
        os.environ["SDA_DP_SINGLE_RANK"] = "1"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
        from speech_decoding_amd import distributed as sd
        sd.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
        sd.emulate_world(N)
        from speech_decoding_amd import loss as _l
        _l.EMULATE_COPY_REMOTE = False
    from speech_decoding_amd.distributed import allreduce_gradients
    enc, lossf, opt, X, Y, plain_step = harness.headline_step()
    params = list(enc.parameters()) + list(lossf.parameters())

    def reduce_grads(phase):                     # bench.py's data-parallel line, between backward and Adam
        if N > 1 and phase == "backward":
            allreduce_gradients(list(lossf.parameters()) if enc.grads_are_reduced else params)

    step = lambda: plain_step(mark=reduce_grads)
    for _ in range(8): step()
    harness.settle()
    print(f"host per step {harness.host_clock(step, 30, 0)[0]:.2f} ms (not profiled)")
    # (backward in the calling thread, so that the profiler sees inside it)
    with torch.autograd.set_multithreading_enabled(False):
        for _ in range(3): step()
        pr = cProfile.Profile(); pr.enable()
        for _ in range(30): step()
        pr.disable(); torch.cuda.synchronize()
    st = pstats.Stats(pr); st.sort_stats("tottime").print_stats(22)
    st.sort_stats("cumtime").print_stats(30)


if __name__ == "__main__":
    main()
