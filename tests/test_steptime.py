"""tools/steptime.py's interleaved timing loop on a scripted clock (CPU): the
order of the calls, the warm-up call, the discarded round, the arithmetic."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "tools"))
from steptime import interleaved_ms  # noqa: E402


class Script:
    """records every call of the forms, of sync and of the clock, in order;
    the clock advances by `cost[name]` seconds per call of form `name`"""

    def __init__(self, cost):
        self.cost, self.log, self.now = cost, [], 0.0
        self.forms = {k: (lambda k=k: self.call(k)) for k in cost}

    def call(self, k):
        self.log.append(k)
        c = self.cost[k]
        self.now += c(len([x for x in self.log if x == k])) if callable(c) else c

    def sync(self):
        self.log.append("sync")

    def clock(self):
        self.log.append("clock")
        return self.now

    def run(self, steps, rounds, **kw):
        return interleaved_ms(self.forms, steps, rounds, sync=self.sync, clock=self.clock, **kw)


@pytest.mark.parametrize("warm", [True, False])
def test_call_order(warm):
    s = Script({"a": 1.0, "b": 2.0})
    s.run(steps=3, rounds=2, warm=warm)
    # round by round, form by form; the clock of a discarded round is never read twice
    one = lambda k, kept: ([k] if warm else []) + ["sync", "clock"] + [k] * 3 + ["sync"] \
        + (["clock"] if kept else [])
    assert s.log == one("a", False) + one("b", False) + one("a", True) + one("b", True)


def test_warm_is_the_default_and_is_not_timed():
    s = Script({"a": 0.5})
    out = s.run(steps=2, rounds=3)
    assert s.log.count("a") == 3 * (1 + 2)
    assert out["a"]["ms"] == 500.0                  # per call: the warm-up call is outside


def test_round_0_is_discarded():
    # the form's first three calls (round 0: warm-up + 2 steps) take 100 s each
    s = Script({"a": lambda n: 100.0 if n <= 3 else 0.25})
    out = s.run(steps=2, rounds=3)
    assert out == {"a": {"ms": 250.0, "range_ms": [250.0, 250.0]}}
    with pytest.raises(ValueError):                 # nothing is left of a single round
        Script({"a": 1.0}).run(steps=1, rounds=1)


def test_median_and_range():
    # 1 + 4 rounds of (warm-up + 2 steps): the timed pairs of rounds 1..4 take
    # 2, 8, 4, 6 ms in all, so 1, 4, 2, 3 ms per call; b is 10x a
    per_round = {1: 1.0, 2: 4.0, 3: 2.0, 4: 3.0}
    cost = lambda scale: lambda n: scale * 1e-3 * per_round.get((n - 1) // 3, 50.0)
    s = Script({"a": cost(1.0), "b": cost(10.0)})
    out = s.run(steps=2, rounds=5)
    assert list(out) == ["a", "b"]
    assert out["a"]["ms"] == pytest.approx(2.5, abs=1e-9)
    assert out["a"]["range_ms"] == pytest.approx([1.0, 4.0], abs=1e-9)
    assert out["b"]["ms"] == pytest.approx(25.0, abs=1e-9)
    assert out["b"]["range_ms"] == pytest.approx([10.0, 40.0], abs=1e-9)
    # rounded to 4 decimals, as the tools' JSON lines always were
    s = Script({"a": 1.23456789e-3})
    assert s.run(steps=1, rounds=2)["a"]["ms"] == 1.2346
