"""tools/: every script imports without running or touching a device, and tools/harness.py schedules its timing forms, refuses
to measure without a GPU and reports a child's status as the sweeps rely on.  No GPU needed."""
import glob
import importlib.util
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
SCRIPTS = sorted(os.path.relpath(p, TOOLS) for p in glob.glob(os.path.join(TOOLS, "**", "*.py"), recursive=True))


def load(rel):
    spec = importlib.util.spec_from_file_location("tools_under_test_" + rel[:-3].replace(os.sep, "_"), os.path.join(TOOLS, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a tool initialised the device at import")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(torch.cuda, "init", refuse)
    monkeypatch.setattr(torch.cuda, "_lazy_init", refuse)
    monkeypatch.syspath_prepend(TOOLS)           # what `python tools/x.py` puts first: the tools find the harness there
    monkeypatch.setattr(sys, "argv", ["tool"])
    return monkeypatch


@pytest.fixture
def harness(no_device):
    return load("harness.py")


def test_there_are_tools():
    assert "harness.py" in SCRIPTS and len(SCRIPTS) > 40


@pytest.mark.parametrize("rel", SCRIPTS)
def test_import_does_nothing(rel, no_device, capsys):
    mod = load(rel)
    if rel != "harness.py":
        assert callable(getattr(mod, "main", None)), f"tools/{rel} has no main()"
    assert capsys.readouterr().out == "", f"tools/{rel} printed at import"


# ------------------------------------------------------------------------------------------------------- stub clock
class Log:
    """A clock whose events number themselves in the order they are recorded, and the log of everything that happened."""

    def __init__(self):
        self.log, self.t = [], 0.0

    def call(self, name):
        return lambda: self.log.append(name)

    def clock(self):
        outer = self

        class Event:
            def record(self):
                outer.t += 1.0
                self.at = outer.t
                outer.log.append("record")

            def synchronize(self):
                outer.log.append("wait")

            def elapsed_time(self, other):
                return other.at - self.at

        def now():
            outer.t += 1.0
            return outer.t
        return types.SimpleNamespace(event=Event, sync=lambda: self.log.append("sync"), now=now)


def calls(log):
    return [x for x in log if x not in ("record", "wait", "sync")]


def test_window_brackets_exactly_iters_calls_after_the_warmup(harness):
    lg = Log()
    ms = harness.window(lg.call("f"), iters=4, warmup=3, clock=lg.clock())
    assert lg.log == ["f"] * 3 + ["sync", "record"] + ["f"] * 4 + ["record", "sync"]
    assert ms == 1.0 / 4                                         # two consecutive records are 1 apart on the stub


def test_rounds_give_one_sample_per_window(harness):
    lg = Log()
    out = harness.rounds(lg.call("f"), iters=2, windows=3, warmup=1, clock=lg.clock())
    assert lg.log == ["f", "sync"] + ["record", "f", "f", "record", "sync"] * 3
    assert out == [0.5, 0.5, 0.5]


@pytest.mark.parametrize("sync_each", [True, False])
def test_alternating_takes_turns_with_reps_calls_per_bracket(harness, sync_each):
    lg = Log()
    fns = [lg.call("f0"), lg.call("f1")]
    out = harness.alternating(fns, iters=3, warmup=2, reps=2, sync_each=sync_each, clock=lg.clock())
    first_record = lg.log.index("record")
    assert lg.log[:first_record] == ["f0", "f1"] * 2 + ["sync"]              # all warm-up calls precede the first timed call
    one = lambda f: ["record", f, f, "record"] + (["wait"] if sync_each else [])
    assert lg.log[first_record:] == (one("f0") + one("f1")) * 3 + ["sync"]
    assert calls(lg.log[first_record:]) == ["f0", "f0", "f1", "f1"] * 3
    assert out == [[0.5] * 3, [0.5] * 3]                                     # one sample list per callable, per call


def test_host_clock_ends_in_a_synchronise(harness):
    lg = Log()
    enqueue, drained = harness.host_clock(lg.call("f"), iters=5, warmup=2, clock=lg.clock())
    assert lg.log == ["f"] * 2 + ["sync"] + ["f"] * 5 + ["sync"]
    assert (enqueue, drained) == (1.0 / 5 * 1e3, 2.0 / 5 * 1e3)              # the stub's clock ticks once per reading


def test_summary(harness):
    s = harness.summarize([3, 1, 2])
    assert (s.n, s.mean, s.median, s.min, s.max) == (3, 2, 2, 1, 3)
    assert harness.us(s) == harness.Summary(3, 2000, 2000, 1000, 3000) and harness.us(0.5) == 500


def test_nothing_is_measured_without_a_gpu(harness):
    f = lambda: None
    entries = [harness.need_gpu, lambda: harness.window(f, 1, 0), lambda: harness.rounds(f, 1, 1, 0),
               lambda: harness.alternating([f], 1, 0), lambda: harness.host_clock(f, 1, 0),
               harness.headline_modules, harness.headline_step]
    for entry in entries:
        with pytest.raises(RuntimeError, match="GPU"):
            entry()


def test_run_child_status(harness):
    assert harness.run_child([sys.executable, "-c", "import sys; sys.exit(3)"], 30) == 3
    assert harness.run_child([sys.executable, "-c", "pass"], 30) == 0
    said = []
    assert harness.run_child([sys.executable, "-c", "print('a'); print('b')"], 30, lines=said) == 0 and said == ["a", "b"]
    status = harness.run_child([sys.executable, "-c", "import time; time.sleep(60)"], 1)
    assert status == harness.TIME_LIMIT and status != 0
    assert harness.child_error(status, 1) == "time limit of 1 s" and harness.child_error(3, 1) == "exit status 3"


def test_emit(harness, tmp_path, capsys):
    out = tmp_path / "sub" / "r.json"
    harness.emit({"a": 1.23456, "b": [2.0, {"c": 0.1234567}]}, str(out), append=True, digits=3)
    harness.emit({"a": 2}, str(out), append=True)
    assert capsys.readouterr().out.splitlines() == ['{"a": 1.235, "b": [2.0, {"c": 0.123}]}', '{"a": 2}']
    assert out.read_text().splitlines() == ['{"a": 1.235, "b": [2.0, {"c": 0.123}]}', '{"a": 2}']
    harness.emit({"a": 2}, str(out))
    assert out.read_text() == '{\n "a": 2\n}\n'
