"""tools/benchlib.py and the bench tools built on it, without a GPU: the summary against the committed records (the records
are the reference, not the code), every touched tool's --help, and the one list of compiler flags.  And tools/kernel_asm.py:
its parser and comparison on a small assembly text, then on the library's device assembly, which is compiled once."""
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
        "policy_minibatch_bench", "gae_bench", "dopri5_bench", "isa_kernel", "isa_diff"]


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


# ------------------------------------------------------------------------------------------------ tools/kernel_asm.py
def _function(name, index, lines, figures, spills):
    """one kernel as the compiler writes it: label, instructions, descriptor directives, comment block"""
    vgpr, agpr, scratch, occ, lds = figures
    text = "\t.text\n\t.globl\t%s\n\t.p2align\t8\n\t.type\t%s,@function\n%s: ; @%s\n; %%bb.0:\n" % (name, name, name, name)
    text += "".join(l + "\n" for l in lines)
    text += ("\t.section\t.rodata,\"a\",@progbits\n\t.p2align\t6, 0x0\n\t.amdhsa_kernel %s\n\t\t.amdhsa_next_free_vgpr %d\n"
             "\t.end_amdhsa_kernel\n\t.text\n.Lfunc_end%d:\n\t.size\t%s, .Lfunc_end%d-%s\n"
             "                                        ; -- End function\n\t.set %s.num_vgpr, %d\n; Kernel info:\n"
             "; codeLenInByte = 64\n; TotalNumSgprs: 20\n; NumVgprs: %d\n; NumAgprs: %d\n; TotalNumVgprs: %d\n; ScratchSize: %d\n"
             "; LDSByteSize: %d bytes/workgroup (compile time only)\n; NumVGPRsForWavesPerEU: %d\n; Occupancy: %d\n"
             % (name, vgpr, index, name, index, name, name, vgpr, vgpr, agpr, vgpr + agpr, scratch, lds, vgpr, occ))
    meta = ("  - .agpr_count:     %d\n    .args:\n      - .offset:         0\n        .size:           8\n"
            "        .value_kind:     global_buffer\n    .group_segment_fixed_size: %d\n    .name:           %s\n"
            "    .private_segment_fixed_size: %d\n    .sgpr_count:     20\n    .sgpr_spill_count: %d\n    .symbol:         %s.kd\n"
            "    .vgpr_count:     %d\n    .vgpr_spill_count: %d\n    .wavefront_size: 64\n"
            % (agpr, lds, name, scratch, spills[0], name, vgpr + agpr, spills[1]))
    return text, meta


FLAT, LOOPY = "_ZN3t1d4flatEPd", "_ZN3t1d5loopyEPdi"
FLAT_LINES = ["\ts_load_dwordx2 s[0:1], s[0:1], 0x0", "\tv_mov_b32_e32 v1, 0 ; a comment", "\ts_waitcnt lgkmcnt(0)",
              "\tglobal_store_dword v1, v0, s[0:1]", "\ts_endpgm"]
LOOPY_LINES = ["\ts_load_dword s2, s[0:1], 0x8", "\ts_getpc_b64 s[4:5]", "\ts_add_u32 s4, s4, _ZN3t1d5tableE@rel32@lo+4",
               "\ts_waitcnt lgkmcnt(0)", "\ts_cmp_lt_i32 s2, 1", "\ts_cbranch_scc1 .LBB7_3", "; %bb.1:", "\tv_mov_b32_e32 v2, 0",
               ".LBB7_2:                                ; =>This Inner Loop Header: Depth=1", "\tds_read_b32 v3, v2",
               "\ts_waitcnt lgkmcnt(0)", "\tv_writelane_b32 v9, s2, 0", "\tscratch_store_dword off, v3, off offset:4",
               "\tds_write_b32 v2, v3", "\ts_add_i32 s2, s2, -1", "\ts_cmp_lg_u32 s2, 0", "\ts_cbranch_scc1 .LBB7_2",
               ".LBB7_3:", "\ts_endpgm"]


def _asm_text(flat_lines=FLAT_LINES, loopy_lines=LOOPY_LINES, order=(0, 1), index="7"):
    parts = [_function(FLAT, 0, flat_lines, (12, 0, 0, 8, 0), (0, 0)),
             _function(LOOPY, 7, loopy_lines, (40, 6, 16, 4, 512), (3, 2))]
    parts = [parts[i] for i in order]
    text = ('\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n' + "".join(p[0] for p in parts) +
            "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(p[1] for p in parts) +
            "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n\n\t.end_amdgpu_metadata\n")
    return text.replace(".LBB7_", ".LBB%s_" % index)


def _parsed(tmp_path, name="a.s", **kw):
    from support import kernel_asm
    path = tmp_path / name
    path.write_text(_asm_text(**kw))
    return kernel_asm().kernels(str(path))


def test_parser_pins_names_figures_and_metadata_of_a_small_text(tmp_path):
    ks = _parsed(tmp_path)
    assert list(ks) == [FLAT, LOOPY]
    assert [k.demangled for k in ks.values()] == ["t1d::flat(double*)", "t1d::loopy(double*, int)"]
    assert ks[FLAT].figures == {"vgprs": 12, "agprs": 0, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 8, "lds_bytes": 0,
                                "sgpr_spill": 0, "vgpr_spill": 0}
    assert ks[LOOPY].figures == {"vgprs": 40, "agprs": 6, "scratch_bytes_per_lane": 16, "occupancy_waves_per_simd": 4,
                                 "lds_bytes": 512, "sgpr_spill": 3, "vgpr_spill": 2}
    assert ks[LOOPY].metadata == {"private_segment_fixed_size": 16, "group_segment_fixed_size": 512, "sgpr_spill_count": 3,
                                  "vgpr_spill_count": 2, "vgpr_count": 46, "agpr_count": 6}
    assert ks[FLAT].body[0].startswith(FLAT + ":") and ks[FLAT].body[2:7] == FLAT_LINES
    assert not any(".Lfunc_end" in l for k in ks.values() for l in k.body)


def test_loop_finder_pins_the_bounds_and_columns_of_the_one_loop(tmp_path):
    from support import kernel_asm
    ks = _parsed(tmp_path)
    assert kernel_asm().loops(ks[FLAT]) == []
    (lp,) = kernel_asm().loops(ks[LOOPY])
    body = ks[LOOPY].body
    assert lp.label == ".LBB7_2" and body[lp.first].startswith(".LBB7_2:") and body[lp.last] == "\ts_cbranch_scc1 .LBB7_2"
    # the seven instructions between the label and the back edge; the forward branch to .LBB7_3 opens no loop
    assert lp[3:] == (7, 1, 1, 1, 1, 1)
    assert lp._fields[3:] == ("instructions", "scratch", "lane_spill", "ds_read", "ds_write", "waitcnt")


def test_instruction_stream_keeps_instructions_and_labels_only(tmp_path):
    from support import kernel_asm
    ks = _parsed(tmp_path)
    assert kernel_asm().instruction_stream(ks[FLAT]) == ["SYM:"] + FLAT_LINES[:1] + ["\tv_mov_b32_e32 v1, 0"] + FLAT_LINES[2:]
    got = kernel_asm().instruction_stream(ks[LOOPY])
    want = ["SYM:"] + [l.split(";")[0].rstrip() for l in LOOPY_LINES if not l.startswith(";")]
    want[3] = "\ts_add_u32 s4, s4, SYM@rel32@lo+4"
    assert got == [l.replace(".LBB7_", ".LBB_") for l in want]


def test_compare_sees_through_label_indices_and_function_order(tmp_path):
    from support import kernel_asm
    compare = kernel_asm().compare
    a = _parsed(tmp_path)
    all_same = [(FLAT, True, 6, 6), (LOOPY, True, 19, 19)]
    assert compare(a, _parsed(tmp_path, "b.s", index="31")) == (all_same, [], [])
    assert ".LBB31_2:" in "\n".join(_parsed(tmp_path, "b.s", index="31")[LOOPY].body)
    swapped = _parsed(tmp_path, "c.s", order=(1, 0))
    assert list(swapped) == [LOOPY, FLAT] and compare(a, swapped) == (all_same, [], [])


def test_compare_reports_one_changed_register_and_a_missing_kernel(tmp_path):
    from support import kernel_asm
    compare = kernel_asm().compare
    a = _parsed(tmp_path)
    changed = [l.replace("ds_read_b32 v3, v2", "ds_read_b32 v4, v2") for l in LOOPY_LINES]
    assert compare(a, _parsed(tmp_path, "d.s", loopy_lines=changed)) == ([(FLAT, True, 6, 6), (LOOPY, False, 19, 19)], [], [])
    one = _parsed(tmp_path, "e.s", order=(0,))
    assert compare(a, one) == ([(FLAT, True, 6, 6)], [LOOPY], [])
    assert compare(one, a) == ([(FLAT, True, 6, 6)], [], [LOOPY])


def test_real_assembly_every_kernel_parsed_and_comment_block_agrees_with_metadata():
    """on the device assembly of the library's sources, the compile the register tests share"""
    from support import kernel_asm
    path = kernel_asm().device_asm()
    ks = kernel_asm().kernels(path)
    assert ks and len(ks) == len(re.findall(r"^\s*\.amdhsa_kernel\s", open(path).read(), re.M))
    for k in ks.values():
        assert k.figures["scratch_bytes_per_lane"] == k.metadata["private_segment_fixed_size"], k.name
        assert k.figures["lds_bytes"] == k.metadata["group_segment_fixed_size"], k.name
        assert k.demangled.startswith("t1d::") or k.demangled.startswith("void t1d::"), k.demangled
    rows, only_a, only_b = kernel_asm().compare(ks, ks)
    assert len(rows) == len(ks) and all(same and n == m and n > 1 for _, same, n, m in rows) and only_a == only_b == []


def test_device_asm_second_call_starts_no_process_and_flags_change_the_name(monkeypatch):
    from support import kernel_asm
    ka = kernel_asm()
    path = ka.device_asm()
    assert os.path.dirname(path) == os.path.join(ROOT, "build") and os.path.getsize(path) > 0

    def refuse(*a, **kw):
        raise AssertionError("a process was started: %r" % (a,))
    for name in ("run", "Popen", "call", "check_call", "check_output"):
        monkeypatch.setattr(subprocess, name, refuse)
    assert ka.device_asm() == path
    other = ka.asm_path(["-O2"])
    assert other != path and os.path.dirname(other) == os.path.dirname(path) and ka.asm_path(["-O2"]) == other
    assert ka.asm_path() == path


def test_dopri5_bench_resources_reads_the_shared_compile():
    """its four keys, equal to the step kernel's entry; dopri5_bench imports torch but asks for no device at import"""
    from support import kernel_asm
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import dopri5_bench
    ks = kernel_asm().kernels(kernel_asm().device_asm())
    (step,) = [k for k in ks.values() if k.name.startswith("_ZN3t1d18dopri5_step_kernel")]
    got = dopri5_bench.resources()
    assert list(got) == ["vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd"]
    assert got == {k: step.figures[k] for k in got}
    (roll,) = [k for k in ks.values() if k.name.startswith("_ZN3t1d21dopri5_rollout_kernel")]
    assert dopri5_bench.resources("_ZN3t1d21dopri5_rollout_kernel") == {k: roll.figures[k] for k in got}


def test_kernel_resources_sh_help_needs_no_compile():
    r = subprocess.run([os.path.join(TOOLS, "kernel_resources.sh"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, env=dict(os.environ, HIPCC="/nonexistent/hipcc"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"usage: kernel_resources.sh" in r.stdout and b"--spills" in r.stdout
