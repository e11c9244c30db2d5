"""Every bench tool that stands on tools/benchlib.py, once, in-process through main([...]) at the smallest shape that walks every
branch of the harness: 128 envs (two waves, both patients), 2 steps or rows, 2 repetitions (alternation and the median), with
and without a warm-up window.  None of this is a measurement: the times are only asked to be positive.  What is checked is
the harness -- the run ends without error, every status is 0, the records have the keys of the committed profiles in their
order, --out holds what was printed, and a leg's repetitions, each on a fresh env from the same seed, end the same share of
episodes."""
import importlib
import json
import os
import sys

import pytest

from support import gpu_torch as _torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--n", "128", "--reps", "2"]
ENV = SMALL + ["--steps", "2"]
# the fields policy_bench.py adds with --exact (its docstring): the plain run's records are exact_bench.json's without them
POLICY_EXACT_ONLY = ("ms_median", "ms_runs", "nfev_mean", "mlp_over_pid")
CASES = {
    "collect": ("collect_bench", ENV + ["--warm-steps", "2"], "collect/collect_bench.json"),
    "collect-cold": ("collect_bench", ENV + ["--warm-steps", "0"], "collect/collect_bench.json"),
    "collect-exact": ("collect_bench", ENV + ["--warm-steps", "2", "--exact"], "collect/exact_collect_bench.json"),
    "ctrl": ("ctrl_collect_bench", ENV + ["--warm-steps", "2"], "collect/ctrl_collect_bench.json"),
    "ctrl-cold": ("ctrl_collect_bench", ENV + ["--warm-steps", "0"], "collect/ctrl_collect_bench.json"),
    "autoreset": ("autoreset_bench", ENV + ["--warmup", "2"], "autoreset/autoreset_bench.json"),
    "policy": ("policy_bench", ENV + ["--warmup", "2"], "policy/exact_bench.json"),
    "policy-exact": ("policy_bench", ENV + ["--warmup", "2", "--exact"], "policy/exact_bench.json"),
    "grad": ("policy_grad_bench", SMALL + ["--rows", "2"], "policy/grad_bench.json"),
    "loss": ("policy_loss_bench", SMALL + ["--rows", "2"], "policy/policy_loss_bench.json"),
    "gae": ("gae_bench", SMALL + ["--rows", "2"], "policy/gae_bench.json"),
    # 2 rows x 128 envs = 4 tiles per policy: B = 1 (with the `plain` leg) and B = 4 (M = 1)
    "minibatch": ("policy_minibatch_bench", SMALL + ["--rows", "2", "--minibatches", "1", "4"], "policy/minibatch_bench.json"),
}


def _shape(rec, drop=()):
    """the keys of a record and of each of its legs, in order"""
    return (tuple(k for k in rec if k not in drop),
            tuple((leg, tuple(k for k in v if k not in drop)) for leg, v in rec.get("legs", {}).items()))


def _times(rec):
    for v in list(rec.get("legs", {}).values()) + [rec]:
        for k, x in v.items():
            if k.endswith(("_median", "_min", "_max")) or k.endswith("_ms") and k != "plain_minus_rollout_ms":
                yield x
            elif k.endswith(("_runs", "_ms_all")) and k != "finish_rate_runs":
                yield from x


@pytest.mark.parametrize("case", sorted(CASES))
def test_tool_runs_and_writes_the_committed_layout(case, tmp_path, capsys, monkeypatch):
    _torch()
    tool, argv, profile = CASES[case]
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    mod = importlib.import_module(tool)
    per_run = []
    if hasattr(mod, "run_leg"):
        run_leg = mod.run_leg

        def recorded(leg, *a):
            # one key per leg and configuration: the policy object stands for itself
            key = (leg,) + tuple(x if isinstance(x, (int, float, str, type(None))) else id(x) for x in a)
            per_run.append((key, run_leg(leg, *a)))
            return per_run[-1][1]
        monkeypatch.setattr(mod, "run_leg", recorded)
    out = tmp_path / "out.json"
    capsys.readouterr()
    mod.main(argv + ["--out", str(out)])
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert printed and printed == json.load(open(out))
    assert [list(r) for r in printed] == [list(r) for r in json.load(open(out))]
    drop = POLICY_EXACT_ONLY if case == "policy" else ()
    committed = {_shape(r, drop) for r in json.load(open(os.path.join(ROOT, "profiles", profile)))}
    for rec in printed:
        assert _shape(rec) in committed, (_shape(rec), committed)
        assert rec.get("n_envs", rec.get("n")) == 128
        times = list(_times(rec))
        assert times and all(t > 0 for t in times), rec
        for leg, v in rec.get("legs", {}).items():
            assert v.get("status", 0) == 0, (leg, v)
            for k in v:
                if k.endswith("_runs"):
                    assert len(v[k]) == 2
    if case == "minibatch":
        assert [(r["minibatches"], r["tiles_per_minibatch"], list(r["legs"])) for r in printed[:2]] == \
            [(1, 4, ["tiles", "gather", "plain"]), (4, 1, ["tiles", "gather"])]
    # the repetitions of a leg: each on a fresh env from the same seed
    for key in ("finish_rate", "restarts_per_env_step"):
        groups = {}
        for config, r in per_run:
            if key in r:
                groups.setdefault(config, []).append(r[key])
        for config, vals in groups.items():
            assert len(vals) == 2 and vals[0] == vals[1], (key, config, vals)
    if case == "collect-exact":
        for rec in printed:
            for v in rec["legs"].values():
                assert len(set(v["finish_rate_runs"])) == 1 and v["finish_rate"] == v["finish_rate_runs"][0]
