#!/usr/bin/env python3
"""Compare two device-assembly files kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include \\
          --cuda-device-only -S photonlibos_amd/csrc/crc32c_device.hip -o head.s
    scripts/kernel_code_diff.py parent.s head.s

The gate of a refactor that shares source between kernels ("The
two-cursor walk, written once"): a kernel whose source did not change must come
out byte-identical, and one whose source did must not have gained a register,
LDS or scratch. Each file is split per kernel symbol, from the symbol's label
to its .Lfunc_end; the numbers of local labels (.LBB12_3, .Lfunc_end12), which
count the functions in front of a kernel, are normalised away. Printed:

  - the kernels present on one side only;
  - how many kernels are byte-identical;
  - for every other kernel the resource values of its kernel descriptor, the
    total instruction count, and every mnemonic whose count differs, each as
    `parent -> head`.

The tool knows no instruction by name: it reports whatever differs. Exit
status: 0 when no resource value grew and no kernel appeared or disappeared,
else 1. CPU only. Compare full-unit builds: the same kernel is compiled
differently in a unit that instantiates fewer of its neighbours.
"""
import collections
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size",
             "group_segment_fixed_size")

_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_END = re.compile(r"^\.Lfunc_end\d+:")
_LOCAL = re.compile(r"(\.L[A-Za-z_]+|\bBB)\d+_(\d+)")  # .LBB12_3, BB12_3, .LJTI12_0: drop the function's number
_FUNC_END = re.compile(r"\.Lfunc_end\d+")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)(?:\s|$)")
_VALUE = re.compile(r"^\s*\.amdhsa_(\w+)\s+(\S+)")


def _normalise(line):
    line = _FUNC_END.sub(".Lfunc_end", line)
    return _LOCAL.sub(r"\1_\2", line)


def kernels(path):
    """{symbol: normalised lines from the symbol's label to its .Lfunc_end}."""
    with open(path) as f:
        lines = f.read().split("\n")
    names = {m.group(1) for m in map(_KERNEL.match, lines) if m}
    out, cur = {}, None
    for line in lines:
        if cur is None:
            m = _LABEL.match(line)
            if m and m.group(1) in names:
                cur = m.group(1)
                out[cur] = [_normalise(line)]
            continue
        out[cur].append(_normalise(line))
        if _END.match(line):
            cur = None
    if cur is not None:
        raise SystemExit(f"{path}: {cur} has no .Lfunc_end")
    missing = names - set(out)
    if missing:
        raise SystemExit(f"{path}: no code found for {sorted(missing)[:3]}")
    return out


def describe(lines):
    """(resource values, instruction count, mnemonic counts) of one kernel."""
    res, ops, descriptor = {}, collections.Counter(), False
    for line in lines:
        if _KERNEL.match(line):
            descriptor = True
        elif line.strip() == ".end_amdhsa_kernel":
            descriptor = False
        elif descriptor:
            m = _VALUE.match(line)
            if m and m.group(1) in RESOURCES:
                res[m.group(1)] = int(m.group(2), 0)
        else:
            m = _INSN.match(line)
            if m:
                ops[m.group(1)] += 1
    return res, sum(ops.values()), ops


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    a, b = kernels(argv[1]), kernels(argv[2])
    bad = False
    for side, only in (("parent", sorted(set(a) - set(b))), ("head", sorted(set(b) - set(a)))):
        for name in only:
            print(f"only in {side}: {name}")
            bad = True
    common = sorted(set(a) & set(b))
    differ = [k for k in common if a[k] != b[k]]
    print(f"{len(a)} kernels in parent, {len(b)} in head; {len(common) - len(differ)} byte-identical, "
          f"{len(differ)} differ")
    for name in differ:
        (ra, na, oa), (rb, nb, ob) = describe(a[name]), describe(b[name])
        print(f"\n{name}")
        for r in RESOURCES:
            grew = rb.get(r, 0) > ra.get(r, 0)
            bad |= grew
            print(f"  {r:28s} {ra.get(r, '-')} -> {rb.get(r, '-')}{'   GREW' if grew else ''}")
        print(f"  {'instructions':28s} {na} -> {nb}")
        for op in sorted(set(oa) | set(ob)):
            if oa[op] != ob[op]:
                print(f"    {op:26s} {oa[op]} -> {ob[op]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
