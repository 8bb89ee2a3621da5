#!/usr/bin/env python3
"""Compare two gfx950 device assembly files (hipcc ... --cuda-device-only -S) kernel by kernel.

    tools/asm_compare.py parent.s new.s [--demangle]

One row per kernel (every function of either file; --demangle prints the C++ names):
    identical                                      the instruction lines are equal, comment text removed
    identical opcode sequence, registers renamed   the mnemonics are equal in order, some operands differ
    differs                                        followed by both sides' VGPRs, SGPRs, SGPR / VGPR spills, scratch bytes, code
                                                   bytes and the counts of the vector and memory instructions that differ
The exit status is 0 whatever the rows say: this tool reports, the reader judges."""
import collections
import re
import subprocess
import sys

# the resource figures of a kernel: its entry in the amdhsa metadata at the end of the file, and the code length of its "Kernel info"
FIGURES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("sgpr_spill", ".sgpr_spill_count"), ("vgpr_spill", ".vgpr_spill_count"),
           ("scratch", ".private_segment_fixed_size"))
# the instruction classes whose counts the residue rule holds equal: vector ALU and every memory instruction
COUNTED = ("v_", "global_", "flat_", "buffer_", "scratch_", "ds_", "s_load_", "s_buffer_load_")


def kernels(path):
    """{name: (instruction lines without comments, {figure: value})} of one assembly file"""
    text = open(path).read().split("\n")
    out, name, last, body = {}, None, None, []
    for ln, line in enumerate(text):
        if name is None:
            m = re.match(r"^(\w+):", line)
            if m and re.match(r"^\s*\.type\s+" + re.escape(m.group(1)) + ",@function", text[ln - 1]):
                name, body = m.group(1), []
            m = re.match(r"^; codeLenInByte = (\d+)", line)
            if m and last:
                out[last][1]["code_bytes"] = int(m.group(1))
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = (body, {})
            name, last = None, name
            continue
        code = line.split(";")[0].strip()
        if code and not code.startswith(".") and not code.endswith(":"):
            body.append(re.sub(r"\s+", " ", code))
    fig = None
    for line in text:
        m = re.match(r"^\s+(\.\w+):\s+(\S+)$", line)
        if m and m.group(1) == ".name":
            fig = out[m.group(2)][1] if m.group(2) in out else None
        elif m and fig is not None:
            fig.update({k: int(m.group(2)) for k, key in FIGURES if key == m.group(1)})
    return out


def verdict(a, b):
    if a == b:
        return "identical"
    if [x.split(" ")[0] for x in a] == [x.split(" ")[0] for x in b]:
        return "identical opcode sequence, registers renamed"
    return "differs"


def counted(body):
    return collections.Counter(op for op in (x.split(" ")[0] for x in body) if op.startswith(COUNTED))


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    ka, kb = kernels(args[0]), kernels(args[1])
    names = sorted(set(ka) | set(kb))
    shown = dict(zip(names, names))
    if "--demangle" in sys.argv and names:
        shown = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")))
    for n in names:
        if n not in ka or n not in kb:
            print(f"{shown[n]}: only in {args[0] if n in ka else args[1]}")
            continue
        (a, fa), (b, fb) = ka[n], kb[n]
        v = verdict(a, b)
        print(f"{shown[n]}: {v}")
        if v == "differs":
            print(f"    parent: {fa}\n    new:    {fb}")
            ca, cb = counted(a), counted(b)
            diff = {op: (ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]}
            print(f"    vector / memory instruction counts that differ (parent, new): {diff if diff else 'none'}")


if __name__ == "__main__":
    main()
