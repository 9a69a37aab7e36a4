"""tools/harness.py on the device: the window and alternating forms around a real launch, and headline_step training."""
import importlib.util
import os

import pytest
import torch

from tests.builders import TOY

pytestmark = pytest.mark.gpu

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


@pytest.fixture(scope="module")
def harness():
    spec = importlib.util.spec_from_file_location("tools_harness_under_test", os.path.join(TOOLS, "harness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_window_and_alternating_on_a_real_launch(harness):
    from speech_decoding_amd import ops
    small = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    large = torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0")
    fns = [lambda: ops.fill_zero_(small), lambda: ops.fill_zero_(large)]
    w_small, w_large = (harness.window(f, 10, 2) for f in fns)
    assert 0 < w_small < w_large
    for samples in (harness.rounds(fns[0], 10, 3, 2), *harness.alternating(fns, 10, 2), *harness.alternating(fns, 10, 2, reps=3, sync_each=False)):
        s = harness.summarize(samples)
        assert s.n == len(samples) and all(x > 0 for x in samples) and s.min <= s.median <= s.max
    a_small, a_large = (harness.summarize(v) for v in harness.alternating(fns, 10, 2))
    assert a_small.n == a_large.n == 10 and len(harness.rounds(fns[0], 10, 3, 2)) == 3
    assert a_large.median > a_small.median
    enqueue, drained = harness.host_clock(fns[1], 10, 2)
    assert 0 < enqueue <= drained


def test_headline_step_trains_at_the_toy_shape(harness):
    before = torch.cuda.current_stream()
    try:
        enc, lossf, opt, X, Y, step = harness.headline_step("bf16", B=8, S=TOY["S"], C=TOY["C"], T=TOY["T"], F=TOY["F"], seed=0)
        assert X.shape == (8, TOY["C"], TOY["T"]) and Y.shape == (8, TOY["F"], TOY["T"])
        start = [p.detach().clone() for p in enc.parameters()]
        seen = []
        losses = [step(), step(mark=seen.append)]
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(l)) for l in losses)
        assert tuple(seen) == harness.PHASES
        assert any(not torch.equal(a, p.detach()) for a, p in zip(start, enc.parameters()))
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(before)                                # headline_step made the training stream current
