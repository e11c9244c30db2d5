"""The library's device assembly, compiled once and parsed in one place: what the register tests, dopri5_bench.resources(),
kernel_resources.sh, isa_kernel.py and isa_diff.py all read.  One `-S --cuda-device-only` compile of csrc/t1d_abi.hip with the
flag list of simglucose_amd/_lib.py holds each kernel's instruction stream (between `NAME:  ; @` and `.Lfunc_end`), its
resource figures (the comment block behind it) and its metadata entry (spill counts).  Importing this compiles nothing."""
import collections
import functools
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from simglucose_amd import _lib  # noqa: E402

TIMEOUT = 900
Kernel = collections.namedtuple("Kernel", "name demangled body figures metadata")
Loop = collections.namedtuple("Loop", "label first last instructions scratch lane_spill ds_read ds_write waitcnt")
# figure -> its key in the comment block behind the function; the two spill counts come from the metadata entry
COMMENT_KEYS = {"vgprs": "NumVgprs", "agprs": "NumAgprs", "scratch_bytes_per_lane": "ScratchSize",
                "occupancy_waves_per_simd": "Occupancy", "lds_bytes": "LDSByteSize"}
METADATA_KEYS = ("private_segment_fixed_size", "group_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count",
                 "vgpr_count", "agpr_count")


def _hipcc():
    return _lib.build_command(os.devnull)[0]


@functools.lru_cache(None)
def _compiler_version(hipcc):
    out = subprocess.run([hipcc, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60).stdout.decode()
    return next(l for l in out.splitlines() if "clang version" in l)


def _sources(root):
    """this checkout's source list under `root` (another checkout: the files of the list that it has)"""
    paths = [os.path.join(root, os.path.relpath(s, ROOT)) for s in _lib.SOURCES]
    return [p for p in paths if os.path.exists(p)]


def asm_path(extra_flags=(), root=ROOT):
    """where device_asm() keeps this content: build/t1d_device_<hash of flags, compiler version line, source bytes>.s"""
    h = hashlib.sha256(repr((_lib.HIPCC_FLAGS + list(extra_flags), _compiler_version(_hipcc()))).encode())
    for s in _sources(root):
        with open(s, "rb") as f:
            h.update(hashlib.sha256(f.read()).digest())
    return os.path.join(ROOT, "build", "t1d_device_%s.s" % h.hexdigest()[:20])


def device_asm(extra_flags=(), root=ROOT):
    """Path of the device assembly of `root`'s sources (this checkout's by default) with the library's flags and
    `extra_flags`, compiled at most once per content: the name is a hash of the content, so a stale file is never looked up
    again.  Built like _lib.build(): under a file lock, into a temporary name, moved into place."""
    import fcntl
    path = asm_path(extra_flags, root)
    if os.path.exists(path):
        return path
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not os.path.exists(path):
                tmp = "%s.tmp.%d" % (path, os.getpid())
                try:
                    r = subprocess.run([_hipcc()] + _lib.HIPCC_FLAGS + list(extra_flags) +
                                       ["-S", "--cuda-device-only", "-o", tmp, _sources(root)[0]],
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=TIMEOUT)
                    if r.returncode:
                        raise RuntimeError("device compile failed:\n" + r.stdout.decode()[-4000:])
                    os.replace(tmp, path)
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return path


def _metadata(text):
    """kernel name -> its fields of METADATA_KEYS from the .amdgpu_metadata section (one `  - .key:` list item per kernel)"""
    at = text.find("\t.amdgpu_metadata")
    out = {}
    for entry in re.split(r"^  - (?=\.)", text[at:] if at >= 0 else "", flags=re.M)[1:]:
        fields = dict(re.findall(r"^(?:    )?\.(\w+): +(\S+)$", entry, re.M))
        if "name" in fields:
            out[fields["name"]] = {k: int(fields[k]) for k in METADATA_KEYS if k in fields}
    return out


def kernels(path):
    """mangled name -> Kernel(name, demangled, body, figures, metadata) of every kernel of the assembly file `path`, in the
    file's order.  body: the lines from `NAME:` up to `.Lfunc_end`; figures: vgprs, agprs, scratch_bytes_per_lane,
    occupancy_waves_per_simd, lds_bytes (comment block) and sgpr_spill, vgpr_spill (metadata)."""
    with open(path) as f:
        text = f.read()
    meta = _metadata(text)
    starts = [m for m in re.finditer(r"^(\w+):\s*; @", text, re.M) if m.group(1) in meta]
    names = [m.group(1) for m in starts]
    demangled = subprocess.run(["c++filt"], input="\n".join(names).encode(), stdout=subprocess.PIPE,
                               check=True).stdout.decode().split("\n") if names else []
    out = {}
    for i, m in enumerate(starts):
        end = text.index(".Lfunc_end", m.end())
        tail = text[end:starts[i + 1].start() if i + 1 < len(starts) else len(text)]
        figures = {k: int(re.search(r"^; %s: (\d+)" % key, tail, re.M).group(1)) for k, key in COMMENT_KEYS.items()}
        figures["sgpr_spill"] = meta[m.group(1)]["sgpr_spill_count"]
        figures["vgpr_spill"] = meta[m.group(1)]["vgpr_spill_count"]
        out[m.group(1)] = Kernel(m.group(1), demangled[i].strip(), text[m.start():end].split("\n"), figures, meta[m.group(1)])
    return out


def is_instruction(line):
    return line.startswith("\t") and line.lstrip()[:1] not in (".", ";", "")


def mnemonics(lines):
    return collections.Counter(l.split()[0] for l in lines if is_instruction(l))


def loops(kernel):
    """The kernel's loops by back edge (a branch to a label above it; the farthest branch closes the loop), outermost first
    in body order.  first / last index kernel.body; the counts are of the instructions in between."""
    body = kernel.body
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    last = {}
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            last[m.group(1)] = i
    out = []
    for label in sorted(last, key=labels.get):
        c = mnemonics(body[labels[label]:last[label]])
        out.append(Loop(label, labels[label], last[label], sum(c.values()), sum(v for k, v in c.items() if "scratch" in k),
                        c["v_readlane_b32"] + c["v_writelane_b32"], sum(v for k, v in c.items() if k.startswith("ds_read")),
                        sum(v for k, v in c.items() if k.startswith("ds_write")), c["s_waitcnt"]))
    return out


NestLoop = collections.namedtuple("NestLoop", "header depth parent children lines")


def loop_nest(kernel):
    """The kernel's loops as the compiler saw them, from the comments it leaves on every basic block (`=>This Loop Header:
    Depth=d`, `Parent Loop BBf_n Depth=d` above it, `in Loop: Header=BBf_n Depth=d` on the other blocks): header label ->
    NestLoop(header, depth, parent header or None, child headers, the body lines of the loop's own blocks -- those of its child
    loops are theirs), in body order.  Unlike loops(), which goes by back edges, a block the layout has moved behind its
    loop's latch still counts to that loop."""
    out, parents, current = {}, [], None
    for l in kernel.body:
        block = re.match(r"(?:\.L(BB\d+_\d+)|; %bb\.\d+):", l)
        if block:
            parents, current = [], None
        m = re.search(r";\s+Parent Loop (BB\d+_\d+) Depth=(\d+)", l)
        if m:
            parents.append(m.group(1))
        m = re.search(r"; =>\s*This (?:Inner )?Loop Header: Depth=(\d+)", l)
        if m:
            # a header's own line either carries the mark or opens the comment block that ends with it
            header = block.group(1) if block else pending
            parent = parents[-1] if parents else None
            out[header] = NestLoop(header, int(m.group(1)), parent, [], [])
            if parent in out:
                out[parent].children.append(header)
            current = header
        if block:
            pending = block.group(1)
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=\d+", l)
            if m:
                current = m.group(1)
        if current in out:
            out[current].lines.append(l)
    return out


def nest_lines(nest, header):
    """the body lines of a loop of loop_nest() with those of every loop inside it"""
    return nest[header].lines + [l for c in nest[header].children for l in nest_lines(nest, c)]


def instruction_stream(kernel):
    """What two builds are compared on: the instruction and label lines without comments, `.LBB<f>_<n>` without the
    function's index f, and every mangled symbol as one token (the kernel's own name in its first line included)."""
    lines = [l.split(";")[0].rstrip() for l in kernel.body]
    text = "\n".join(l for l in lines if is_instruction(l) or (l.endswith(":") and l[0] not in " \t"))
    return re.sub(r"\b_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", text)).split("\n")


def compare(kernels_a, kernels_b):
    """([(name, same, len_a, len_b) for the names on both sides, in a's order], names only in a, names only in b)"""
    rows = []
    for name in kernels_a:
        if name in kernels_b:
            a, b = instruction_stream(kernels_a[name]), instruction_stream(kernels_b[name])
            rows.append((name, a == b, len(a), len(b)))
    return rows, [n for n in kernels_a if n not in kernels_b], [n for n in kernels_b if n not in kernels_a]


def select(ks, pattern):
    """the kernels whose mangled name contains `pattern` or whose demangled name matches it as a regex"""
    return [k for k in ks.values() if pattern in k.name or re.search(pattern, k.demangled)]


def main(argv):
    """tools/kernel_resources.sh"""
    import argparse
    ap = argparse.ArgumentParser(prog="kernel_resources.sh", description="One line per kernel whose demangled name matches "
                                 "PATTERN: NAME vgpr V agpr A scratch S occ O lds L (scratch in bytes per lane, occ in waves per "
                                 "SIMD, lds in static bytes per workgroup).  Anything else is passed to hipcc behind the library's flags.")
    ap.add_argument("pattern", nargs="?", default=".", help="regex on the demangled name (default: every kernel)")
    ap.add_argument("--spills", action="store_true", help="append sgpr_spill N vgpr_spill M from the kernel's metadata")
    a, flags = ap.parse_known_args(argv)
    for k in kernels(device_asm(flags)).values():
        if re.search(a.pattern, k.demangled):
            f = k.figures
            print(k.demangled, "vgpr", f["vgprs"], "agpr", f["agprs"], "scratch", f["scratch_bytes_per_lane"], "occ",
                  f["occupancy_waves_per_simd"], "lds", f["lds_bytes"],
                  *(("sgpr_spill", f["sgpr_spill"], "vgpr_spill", f["vgpr_spill"]) if a.spills else ()))


if __name__ == "__main__":
    main(sys.argv[1:])
