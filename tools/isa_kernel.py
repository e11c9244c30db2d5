#!/usr/bin/env python3
"""Static look at a kernel's ISA in the device assembly of tools/kernel_asm.py: the instruction mix; per loop of 100
instructions and more (by back edge) the instruction, scratch (VGPR spill), v_readlane/v_writelane (SGPR spill), LDS and wait
counts; and the line numbers of every scratch instruction, so that spills can be told apart by where they sit (around an
integration loop: paid per minute; in a rare branch: free).  Line numbers count from the kernel's own first line (-o FILE)."""
import argparse
import sys

import kernel_asm


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, epilog="Anything else is passed to hipcc behind the library's flags.")
    ap.add_argument("pattern", help="substring of the mangled name, or regex on the demangled name")
    ap.add_argument("-o", metavar="FILE", help="write the (last) matching kernel's assembly here")
    a, flags = ap.parse_known_args(argv)
    for k in kernel_asm.select(kernel_asm.kernels(kernel_asm.device_asm(flags)), a.pattern):
        if a.o:
            with open(a.o, "w") as f:
                f.write("\n".join(k.body))
        c = kernel_asm.mnemonics(k.body)
        print(k.demangled)
        print("  instructions %d  fp64 fma/mul/add %d  ds_read %d  s_waitcnt %d  scratch %d  readlane/writelane %d" % (
            sum(c.values()), c["v_fma_f64"] + c["v_fmac_f64_e32"] + c["v_mul_f64"] + c["v_add_f64"],
            sum(v for m, v in c.items() if m.startswith("ds_read")), c["s_waitcnt"], sum(v for m, v in c.items() if "scratch" in m),
            c["v_readlane_b32"] + c["v_writelane_b32"]))
        for lp in kernel_asm.loops(k):
            if lp.instructions >= 100:
                print("  loop %-10s lines %5d-%5d instrs %5d scratch %3d lane-spill %3d ds_read %3d ds_write %3d waitcnt %3d" % lp)
        print("  scratch at lines:", [i for i, l in enumerate(k.body) if kernel_asm.is_instruction(l) and "scratch" in l.split()[0]])


if __name__ == "__main__":
    main(sys.argv[1:])
