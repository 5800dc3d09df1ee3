"""CPU tests of _optim.GraphRunner (warm-up -> one capture attempt -> replay) with stand-ins for the HIP graphs."""
import contextlib
import warnings

import pytest
import torch


class Harness:
    """Three counted stages (the middle one a collective: stays eager) and a torch.cuda.graph / CUDAGraph that only count."""

    def __init__(self, monkeypatch, warmup, capture_raises=False):
        import sqfa_amd._optim as opt
        self.calls = {"a": 0, "collective": 0, "b": 0}
        self.captures, self.replays, self.calls_at_first_capture = [], 0, None
        harness = self

        class FakeGraph:
            def pool(self):
                return ("pool of", id(self))

            def replay(self):
                harness.replays += 1

        @contextlib.contextmanager
        def fake_capture(g, pool=None, **options):
            if harness.calls_at_first_capture is None:
                harness.calls_at_first_capture = dict(harness.calls)
            harness.captures.append((g, pool, options))
            if capture_raises:
                raise RuntimeError("no capture here")
            yield

        monkeypatch.setattr(opt, "GRAPH_WARMUP_CLOSURES", warmup)
        monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
        monkeypatch.setattr(torch.cuda, "graph", fake_capture)
        self.box = {}
        stages = [lambda n=n: self.calls.__setitem__(n, self.calls[n] + 1) for n in ("a", "collective", "b")]
        self.runner = opt.GraphRunner(stages, self.box, eager_stages=(1,), what="test closure", capture_error_mode="thread_local")


@pytest.mark.parametrize("warmup", [0, 1, 3])
def test_exactly_the_warmup_closures_run_before_the_capture_and_collectives_run_on_every_replay(monkeypatch, warmup):
    h = Harness(monkeypatch, warmup)
    for _ in range(warmup + 4):
        assert h.runner.run() is h.box
    assert h.calls_at_first_capture == {"a": warmup, "collective": warmup, "b": warmup}
    assert h.runner.state == "on" and h.runner.calls == warmup
    # one capture: every graphed stage once, in one shared pool, with the requested error mode; never again
    (g0, pool0, opt0), (g1, pool1, opt1) = h.captures
    assert pool0 is None and pool1 == g0.pool() and opt0 == opt1 == {"capture_error_mode": "thread_local"}
    assert [g is not None for g in h.runner.graphs] == [True, False, True]
    # 4 runs after the warm-up: the first captures (stage bodies run once more, inside the capture) and replays
    assert h.calls["a"] == h.calls["b"] == warmup + 1
    assert h.replays == 2 * 4                              # two graphs per evaluation
    assert h.calls["collective"] == warmup + 1 + 4         # eager during the capture and on EVERY replay


def test_a_failed_capture_warns_once_and_stays_eager(monkeypatch):
    h = Harness(monkeypatch, 2, capture_raises=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(6):
            h.runner.run()
    assert len(caught) == 1 and "HIP graph capture of the test closure failed (no capture here); running eagerly" in str(caught[0].message)
    assert len(h.captures) == 1 and h.runner.state == "eager" and h.runner.graphs is None and h.replays == 0
    assert h.calls == {"a": 6, "collective": 6, "b": 6}


def test_an_unarmed_runner_never_captures(monkeypatch):
    import sqfa_amd._optim as opt
    h = Harness(monkeypatch, 0)
    runner = opt.GraphRunner(h.runner.stages, h.box, armed=False)
    for _ in range(3):
        runner.run()
    assert h.captures == [] and runner.state == "eager" and h.calls["a"] == 3
