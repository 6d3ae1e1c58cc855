"""tools/rates_support.py on the CPU: the measurement protocol every tools/*_rates.py quotes its rates from, on stand-in env batches
whose timing_end returns scripted milliseconds and which record every call; and the row writer."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("rates_support", os.path.join(ROOT, "tools", "rates_support.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


class FakeEnv:
    """timing_begin / timing_end of an env batch: logs both, hands out the scripted window times in order"""

    def __init__(self, name, log, ms):
        self.name, self.log, self.ms = name, log, iter(ms)

    def timing_begin(self):
        self.log.append(self.name + " begin")

    def timing_end(self):
        self.log.append(self.name + " end")
        return next(self.ms), 0


def _window(env, call, inner):
    return [env + " begin"] + [call] * inner + [env + " end", "sync"]


def test_rounds_alternate_and_the_warm_up_is_dropped():
    log = []
    ea, eb = FakeEnv("ea", log, [100.0, 9.0, 3.0, 6.0]), FakeEnv("eb", log, [200.0, 40.0, 10.0, 20.0])
    arms = [R.Arm(lambda: log.append("a"), ea, 3), R.Arm(lambda: log.append("b"), eb)]
    t_a, t_b = R.alternate(arms, rounds=3, warmup=1, sync=lambda: log.append("sync"))
    # four rounds of A then B, each call inside its own env's window, one synchronise after every window and nowhere else
    assert log == (_window("ea", "a", 3) + _window("eb", "b", 1)) * 4
    # the first round's 100 and 200 ms are gone; a window is divided by its calls
    assert t_a == [3.0, 1.0, 2.0] and t_b == [40.0, 10.0, 20.0]
    assert R.median(t_a) == 2.0 and R.median(t_b) == 20.0 and isinstance(R.median(t_a), float)
    assert R.spread(t_a, t_b) == [1.0, 3.0, 10.0, 40.0]


def test_no_warm_up_and_one_arm():
    log = []
    env = FakeEnv("e", log, [8.0, 4.0])
    (t,) = R.alternate([R.Arm(lambda: log.append("x"), env, 4)], rounds=2, warmup=0, sync=lambda: log.append("sync"))
    assert t == [2.0, 1.0] and log == _window("e", "x", 4) * 2


def test_a_plain_callable_runs_between_the_arms_outside_every_window():
    log = []
    env = FakeEnv("e", log, [1.0, 2.0, 3.0, 4.0])
    t_a, t_b = R.alternate([R.Arm(lambda: log.append("a"), env), lambda: log.append("hook"), R.Arm(lambda: log.append("b"), env)],
                           rounds=1, sync=lambda: log.append("sync"))
    assert log == (_window("e", "a", 1) + ["hook"] + _window("e", "b", 1)) * 2          # (the warm-up round runs it too)
    assert t_a == [3.0] and t_b == [4.0]


def test_row_writer_truncates_once_then_appends(tmp_path, capsys):
    out = tmp_path / "sub" / "rates.jsonl"
    out.parent.mkdir()
    out.write_text("stale\n")
    write = R.row_writer(str(out))
    assert out.read_text() == ""
    rows = [dict(family="cube", M=1, ms=0.5), dict(family="go2flat", M=2, ms=0.25)]
    for row in rows:
        write(row)
    lines = out.read_text().splitlines()
    assert [json.loads(l) for l in lines] == rows and [list(json.loads(l)) for l in lines] == [list(r) for r in rows]
    assert capsys.readouterr().out.splitlines() == lines
    # no file: prints only; a missing directory is made
    R.row_writer(None)(rows[0])
    assert capsys.readouterr().out.splitlines() == lines[:1]
    R.row_writer(str(tmp_path / "new" / "r.jsonl"))(rows[1])
    assert (tmp_path / "new" / "r.jsonl").read_text().splitlines() == lines[1:]
