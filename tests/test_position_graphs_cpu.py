"""decode.PositionGraphs — "a position's kernel sequence, eager once, then a captured graph" — without a device: a stub stands in for
ops.Graph and records captures and launches, a counting function stands in for the kernel sequence. The sequences asserted are
those of the three policies the decode side has: DecodePlan's (position 0 warms nothing), BeamSearch's, and the samplers'
(capture_behind, one lane for the unconstrained and one for the constrained keys)."""
import types

import pytest

from musicstyletransfer_amd import decode


class Recorder:
    """the event log of one runner: ('E', key) an eager run, ('C', key) a capture (the stub runs fn once, as ops.Graph.capture does),
    ('L', key) a replay"""

    def __init__(self, monkeypatch, use_graphs, capture_behind=False):
        self.log, self.fn_calls, self.capturing = [], 0, False
        rec = self

        class Graph:
            def capture(self, fn):
                rec.capturing = True
                fn()
                rec.capturing = False
                self.key = rec.log[-1][1]
                return self

            def launch(self):
                rec.log.append(("L", self.key))

        monkeypatch.setattr(decode.o, "Graph", Graph)
        self.plan = types.SimpleNamespace(use_graphs=use_graphs)
        self.runner = decode.PositionGraphs(self.plan, capture_behind=capture_behind)

    def fn(self, key):
        def run():
            self.fn_calls += 1
            self.log.append(("C" if self.capturing else "E", key))
        return run

    def drive(self, keys, lane=False, warms=lambda key: True):
        """one run over `keys`; -> its events"""
        start = len(self.log)
        for key in keys:
            self.runner.run(key, self.fn(key), lane=lane, warms=warms(key))
        return self.log[start:]

    @property
    def keys(self):
        return set(self.runner.graphs)


def E(*keys):
    return [("E", k) for k in keys]


def CL(*keys):  # captured at first use, then launched
    return [ev for k in keys for ev in (("C", k), ("L", k))]


def L(*keys):
    return [("L", k) for k in keys]


def test_the_graphs_dict_is_a_plain_dict_of_the_runner(monkeypatch):
    r = Recorder(monkeypatch, True)
    assert type(r.runner.graphs) is dict and r.runner.graphs == {} and r.runner.warm == set()


def test_decode_plan_policy(monkeypatch):
    """DecodePlan._run_position: key t, warms = (t >= 1) — position 0 touches only the layers' kernels, so it warms nothing; an
    eager position is not captured in that run"""
    r = Recorder(monkeypatch, True)
    warms = lambda t: t >= 1
    assert r.drive(range(5), warms=warms) == E(0, 1) + CL(2, 3, 4)
    assert r.keys == {2, 3, 4} and r.fn_calls == 5
    assert r.drive(range(5), warms=warms) == CL(0, 1) + L(2, 3, 4)
    assert r.keys == {0, 1, 2, 3, 4} and r.fn_calls == 7
    assert r.drive(range(5), warms=warms) == L(0, 1, 2, 3, 4)
    assert r.fn_calls == 7  # a replay never runs fn


def test_a_plan_that_only_ever_runs_position_0_stays_eager(monkeypatch):
    """the samplers' own plans: plan._run_position(0) and nothing else"""
    r = Recorder(monkeypatch, True)
    for _ in range(3):
        assert r.drive([0], warms=lambda t: t >= 1) == E(0)
    assert r.keys == set() and r.fn_calls == 3


def test_beam_search_policy(monkeypatch):
    """BeamSearch.run: key i >= 1, the first position ever eager and captured by the next run"""
    r = Recorder(monkeypatch, True)
    assert r.drive(range(1, 5)) == E(1) + CL(2, 3, 4)
    assert r.keys == {2, 3, 4} and r.fn_calls == 4
    assert r.drive(range(1, 5)) == CL(1) + L(2, 3, 4)
    assert r.keys == {1, 2, 3, 4} and r.fn_calls == 5
    assert r.drive(range(1, 3)) == L(1, 2) and r.fn_calls == 5  # (a run that stops early)


def test_sampler_policy_captures_behind_the_eager_position(monkeypatch):
    """FrameSampling / TokenSampling: keys (i, tau, ...) and (i, tau, ..., True), lane = held"""
    r = Recorder(monkeypatch, True, capture_behind=True)
    free = [(i, 1.0, "draw", 0.5) for i in range(1, 5)]
    # the eager position is captured behind its eager run and NOT launched (it has run already)
    assert r.drive(free) == E(free[0]) + [("C", free[0])] + CL(*free[1:])
    assert r.keys == set(free) and r.fn_calls == 5
    graphs = dict(r.runner.graphs)
    assert r.drive(free) == L(*free)                       # the second run adds nothing
    assert r.keys == set(free) and r.fn_calls == 5
    # a constrained run: its own lane is cold, so its first position is eager again; the key set doubles
    held = [k + (True,) for k in free]
    assert r.drive(held, lane=True) == E(held[0]) + [("C", held[0])] + CL(*held[1:])
    assert r.keys == set(free) | set(held) and len(r.keys) == 2 * len(free) and r.fn_calls == 10
    assert all(r.runner.graphs[k] is graphs[k] for k in free)  # the unconstrained keys are as they were
    assert r.drive(held, lane=True) == L(*held) and r.drive(free) == L(*free)
    assert len(r.keys) == 2 * len(free) and r.fn_calls == 10
    # another tau adds its own keys; its lane is warm, so nothing runs eagerly
    other = [(i, 0.5, "draw", 0.5) for i in range(1, 5)]
    assert r.drive(other) == CL(*other)
    assert r.keys == set(free) | set(held) | set(other) and r.fn_calls == 14
    assert r.drive(other) == L(*other) and r.fn_calls == 14


@pytest.mark.parametrize("capture_behind", [False, True])
def test_graphs_off_no_key_ever(monkeypatch, capture_behind):
    r = Recorder(monkeypatch, False, capture_behind=capture_behind)
    for n in (1, 2):
        assert r.drive(range(5), warms=lambda t: t >= 1) == E(0, 1, 2, 3, 4)
        assert r.drive(range(1, 5)) == E(1, 2, 3, 4)
        assert r.drive([(i, 1.0, True) for i in range(1, 5)], lane=True) == E(*[(i, 1.0, True) for i in range(1, 5)])
        assert r.keys == set() and r.fn_calls == 13 * n


def test_use_graphs_is_read_at_every_position(monkeypatch):
    r = Recorder(monkeypatch, True)
    r.drive(range(1, 5))
    r.drive(range(1, 5))
    r.plan.use_graphs = False
    assert r.drive(range(1, 6)) == E(1, 2, 3, 4, 5) and r.keys == {1, 2, 3, 4}
    r.plan.use_graphs = True
    assert r.drive(range(1, 6)) == L(1, 2, 3, 4) + CL(5)
