#!/usr/bin/env python3
"""Did the kernels move?  Compares every kernel's instruction stream (kernel_asm.instruction_stream: block labels renumbered,
comments and directives dropped) in this checkout's device assembly with OTHER's: one DIFF line per kernel that differs, the
kernels on one side only, and `same N diff M`.  OTHER is another checkout's root (its sources, this checkout's flags and source
list) or an assembly file from `hipcc -S --cuda-device-only`."""
import argparse
import os
import sys

import kernel_asm


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, epilog="Anything else is passed to hipcc behind the library's flags, on both sides.")
    ap.add_argument("other", metavar="OTHER", help="another checkout's root, or an assembly file")
    a, flags = ap.parse_known_args(argv)
    mine = kernel_asm.kernels(kernel_asm.device_asm(flags))
    other = kernel_asm.kernels(kernel_asm.device_asm(flags, root=os.path.abspath(a.other)) if os.path.isdir(a.other) else a.other)
    rows, only_mine, only_other = kernel_asm.compare(mine, other)
    for name, same, n_mine, n_other in rows:
        if not same:
            print("DIFF", n_mine, n_other, mine[name].demangled)
    for side, names, ks in (("here", only_mine, mine), ("OTHER", only_other, other)):
        for name in names:
            print("only in", side, ks[name].demangled)
    print("same", sum(r[1] for r in rows), "diff", sum(not r[1] for r in rows))
    return rows, only_mine, only_other


if __name__ == "__main__":
    main(sys.argv[1:])
