"""tools/ctrl_collect_bench.py --exact, once, in-process at the smallest shape that walks its four legs (the pattern of
test_gpu_tools.py): 128 envs, 2 steps, 2 repetitions.  No measurement: the run ends, every status is 0, the times are positive,
the records have the keys of profiles/collect/exact_ctrl_collect_bench.json in their order, and --out holds what was printed."""
import importlib
import json
import os

import pytest

from support import gpu_torch as _torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shape(rec):
    return tuple(rec), tuple((leg, tuple(v)) for leg, v in rec["legs"].items())


def test_exact_legs_run_and_write_the_committed_layout(tmp_path, capsys, monkeypatch):
    _torch()
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    mod = importlib.import_module("ctrl_collect_bench")
    out = tmp_path / "out.json"
    capsys.readouterr()
    mod.main(["--n", "128", "--reps", "2", "--steps", "2", "--warm-steps", "2", "--exact", "--out", str(out)])
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(printed) == 2 and printed == json.load(open(out))
    committed = {_shape(r) for r in json.load(open(os.path.join(ROOT, "profiles", "collect", "exact_ctrl_collect_bench.json")))}
    for rec in printed:
        assert _shape(rec) in committed, (_shape(rec), committed)
        assert rec["n_envs"] == 128 and rec["integrator"] == "dopri5" and list(rec["legs"]) == ["collect", "loop", "plain", "rollout"]
        assert rec["loop_over_collect"] > 0 and rec["plain_over_rollout"] > 0
        for leg, v in rec["legs"].items():
            assert v["status"] == 0, (leg, v)
            assert len(v["ms_runs"]) == 2 and all(t > 0 for t in v["ms_runs"]) and v["ms_min"] <= v["ms_median"] <= v["ms_max"]
            assert len(set(v["finish_rate_runs"])) == 1 and v["finish_rate"] == v["finish_rate_runs"][0]
