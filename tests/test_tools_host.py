"""tools/benchlib.py and the bench tools built on it, without a GPU: the summary against the committed records (the records
are the reference, not the code), every touched tool's --help, and the one list of compiler flags."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
RECORDS = ["collect/collect_bench.json", "collect/exact_collect_bench.json", "collect/ctrl_collect_bench.json",
           "autoreset/autoreset_bench.json", "policy/exact_bench.json", "policy/grad_bench.json", "policy/policy_loss_bench.json"]
# what each tool computes from its legs' medians alone (m: leg -> median of the tool's first figure)
RATIOS = {"loop_over_collect": lambda m: m["loop"] / m["collect"],
          "plain_over_rollout": lambda m: m["plain"] / m["rollout"],
          "plain_minus_rollout_ms": lambda m: m["plain"] - m["rollout"],
          "host_over_mlp": lambda m: m["host"] / m["mlp"],
          "net_share": lambda m: 1.0 - m["pid"] / m["mlp"],
          "mlp_over_pid": lambda m: m["mlp"] / m["pid"],
          "autograd_over_device": lambda m: m["autograd"] / m["device"],
          "torch_over_fused": lambda m: m["torch"] / m["fused"]}
HELP = ["collect_bench", "ctrl_collect_bench", "autoreset_bench", "policy_bench", "policy_grad_bench", "policy_loss_bench",
        "policy_minibatch_bench", "gae_bench", "dopri5_bench"]


def _benchlib():
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import benchlib
    return benchlib


@pytest.mark.parametrize("name", RECORDS)
def test_summarise_gives_the_committed_medians_and_ratios(name):
    summarise = _benchlib().summarise
    records = json.load(open(os.path.join(ROOT, "profiles", name)))
    assert records
    seen = set()
    for rec in records:
        first = {}
        for leg, v in rec["legs"].items():
            figures = [k[:-len("_runs")] for k in v if k.endswith("_runs") and k[:-len("_runs")] + "_median" in v]
            assert figures, (name, leg)
            for fig in figures:
                spread = fig + "_min" in v
                got = summarise(v[fig + "_runs"], fig, spread=spread)
                assert list(got) == [fig + "_median"] + ([fig + "_min", fig + "_max"] if spread else []) + [fig + "_runs"]
                assert got == {k: v[k] for k in got}, (name, leg, fig)
            first[leg] = v[figures[0] + "_median"]
        for key in RATIOS:
            if key in rec:
                assert RATIOS[key](first) == rec[key], (name, key)      # bit-equal: the same expression on the same medians
                seen.add(key)
    assert seen or name == "autoreset/autoreset_bench.json"             # the one tool that reports no ratio


def test_summarise_takes_the_upper_median_and_leaves_its_input_alone():
    summarise = _benchlib().summarise
    runs = [3.0, 1.0, 4.0, 2.0]
    assert summarise(runs, "ms", spread=True) == {"ms_median": 3.0, "ms_min": 1.0, "ms_max": 4.0, "ms_runs": [3.0, 1.0, 4.0, 2.0]}
    assert runs == [3.0, 1.0, 4.0, 2.0]
    assert summarise([5.0], "us") == {"us_median": 5.0, "us_runs": [5.0]}


@pytest.mark.parametrize("tool", HELP)
def test_help_needs_no_device(tool):
    """imports the tool and benchlib, parses, exits 0: nothing before parse_args may ask for a device"""
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool + ".py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"usage" in r.stdout


def test_no_tool_imports_a_sibling_bench_and_the_exact_collect_bench_is_gone():
    assert not os.path.exists(os.path.join(TOOLS, "collect_exact_bench.py"))
    for f in sorted(os.listdir(TOOLS)):
        if f.endswith(".py"):
            assert not re.search(r"^\s*(from|import)\s+(tools\.)?\w*_bench\b", open(os.path.join(TOOLS, f)).read(), re.M), f


def test_the_build_command_carries_the_exported_flag_list():
    from simglucose_amd import _lib
    flags = _lib.HIPCC_FLAGS
    assert flags and all(isinstance(f, str) and f.startswith("-") for f in flags)
    for verbose in (False, True):
        cmd = _lib.build_command("out.so", verbose)
        at = cmd.index(flags[0])
        assert cmd[at:at + len(flags)] == flags
        assert cmd[-3:] == ["-o", "out.so", _lib.SOURCES[0]] and "-shared" in cmd
