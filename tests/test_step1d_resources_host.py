"""Compile only: step1d_kernel, the single-minute launch with the refinement set aside, runs four waves per SIMD in both
precisions, and in fp64 -- where that means 128 VGPRs for a main pass that used 168 -- nothing is spilled where it would
be paid per sub-step: the innermost loops of the main chunk loop hold no scratch access.  Read from the one device compile
that the register tests share (tools/kernel_asm.py)."""
import re

import pytest

from support import kernel_asm


@pytest.fixture(scope="module")
def step1d():
    """demangled template arguments, e.g. "double, false" -> Kernel"""
    ka = kernel_asm()
    ks = ka.kernels(ka.device_asm())
    out = {}
    for k in ks.values():
        m = re.match(r"void t1d::step1d_kernel<(\w+, \w+)>\(", k.demangled)
        if m:
            out[m.group(1)] = k
    assert sorted(out) == ["double, false", "double, true", "float, false", "float, true"]
    return out


def _scratch(lines):
    ka = kernel_asm()
    return sum(v for k, v in ka.mnemonics(lines).items() if "scratch" in k)


def _main_chunk_loop(nest):
    """the first loop of the kernel that holds other loops: staging has none, the pass over the list comes behind it"""
    return next(l for l in nest.values() if l.depth == 1 and l.children)


@pytest.mark.parametrize("inst", ["double, false", "double, true", "float, false", "float, true"])
def test_four_waves_per_simd(step1d, inst):
    f = step1d[inst].figures
    print(inst, f)
    assert f["occupancy_waves_per_simd"] == 4 and f["vgprs"] <= 128 and f["agprs"] == 0


@pytest.mark.parametrize("inst", ["double, false", "double, true"])
def test_no_scratch_in_the_innermost_loops_of_the_main_chunk_loop(step1d, inst):
    ka = kernel_asm()
    k = step1d[inst]
    nest = ka.loop_nest(k)
    main = _main_chunk_loop(nest)

    def leaves(h):
        return [h] if not nest[h].children else [x for c in nest[h].children for x in leaves(c)]
    inner = leaves(main.header)
    # the sub-step loop of the glucose sub-system is among them: by far the longest, all of it fp64 arithmetic
    sizes = {h: sum(ka.mnemonics(nest[h].lines).values()) for h in inner}
    fma = {h: sum(v for m, v in ka.mnemonics(nest[h].lines).items() if m.startswith("v_fma_f64")) for h in inner}
    print(inst, "main chunk loop", main.header, "scratch accesses in all of it:", _scratch(ka.nest_lines(nest, main.header)),
          "innermost loops (instructions):", sizes)
    assert max(sizes.values()) > 300 and max(fma.values()) > 100
    for h in inner:
        assert _scratch(nest[h].lines) == 0, (h, [l for l in nest[h].lines if "scratch" in l])
