"""Instruction ledger of the production extend kernel's traversal loops.

usage: python tools/extend_ledger.py [--kernel MANGLED] [hipcc flags...]

Compiles path-tracer_amd/csrc/hip/extend.hip device-only to assembly with
build.py's flags plus the flags given, takes one kernel (default: the
renderer's mesh-only instantiation with the u16 stack, the node cache and the
RUN block map) and counts, per basic block of each traversal loop, the VALU,
SALU, vector-memory and LDS instructions.  A block is named by what it holds:

  face      the face test (three 16-byte loads of one face, the vertex pack)
  divide    the IEEE division beside the fast reciprocal
  node      the child pair's loads (global or LDS copy)
  box       the two slab tests
  push/pop  the stack write / read
  hit       the hit-state selects
  join      everything else between the halves and the loop's end

and a wave step's cost on a path is the sum of the blocks that path enters
(every block is entered by a wave with at least one lane on it).  The loop
whose box block divides is the IEEE one; the other is the exact fast division
loop nearly every ray takes.  DESIGN.md §4 "Lean extend" quotes the table.
"""
from __future__ import annotations

import importlib.util
import re
import subprocess
import sys
import tempfile
from collections import OrderedDict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pt_build", ROOT / "path-tracer_amd" / "build.py")
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)

KERNEL = "_ZN3ptd13extend_kernelINS_16ray_source_slotsELb0ELi5ELi20EtLb1ELb1ELb0ELb1EEEvNS_6dsceneET_jPjj"


def assembly(flags):
    with tempfile.TemporaryDirectory(prefix="extend_ledger_") as tmp:
        out = Path(tmp) / "extend.s"
        subprocess.run([build.HIPCC, *build.hip_flags(flags), "--cuda-device-only", "-S", "-o", str(out),
                        str(ROOT / "path-tracer_amd" / "csrc" / "hip" / "extend.hip")], check=True,
                       stderr=subprocess.DEVNULL)
        return out.read_text()


def kernel_text(text, name):
    lines, on = [], False
    for line in text.splitlines():
        if line.startswith(name + ":"):
            on = True
        if on:
            lines.append(line)
            if line.startswith(".Lfunc_end"):
                break
    if not lines:
        sys.exit(f"kernel {name} not in extend.hip's assembly")
    return lines


def resources(text, name):
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S)
    out = {}
    for key in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size"):
        v = re.search(r"\.amdhsa_" + key + r" (\d+)", m.group(1)) if m else None
        out[key] = int(v.group(1)) if v else None
    return out


def kind(op):
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return None


def name_block(ops):
    has = lambda p: any(o.startswith(p) for o in ops)
    if sum(o.startswith("global_load_dwordx4") for o in ops) == 3 or (has("v_rcp_f32") and not has("v_max3_f32") and not has("v_div_scale")):
        return "face"
    if has("v_max3_f32"):
        return "box"
    if has("v_min3_f32"):
        return "face"   # the part of the face test behind the division block
    if has("v_div_scale"):
        return "divide"
    if has("ds_write_b16") or has("ds_write_b32"):
        return "push"
    if has("ds_read_u16") or has("ds_read_b32"):
        return "pop"
    if has("global_load_dwordx4") or has("ds_read_b128"):
        return "node"
    if sum(o.startswith("v_cndmask") for o in ops) >= 8:
        return "hit"
    return "join"


def loops(lines):
    """{loop header label: [(block label, [opcodes])]} of the kernel's inner loops."""
    out, cur, hdr = OrderedDict(), None, None
    for line in lines:
        m = re.match(r"^(\.LBB\d+_\d+):|^; %(bb\.\d+):", line)
        if m:
            label = m.group(1) or m.group(2)
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", line)
            if "This Inner Loop Header" in line:
                hdr = label.lstrip(".L")
            elif h:
                hdr = h.group(1)
            else:
                hdr = None
            cur = None
            if hdr is not None:
                cur = []
                out.setdefault(hdr, []).append((label, cur))
            continue
        if cur is not None and line.startswith("\t") and not line.startswith("\t;"):
            op = line.split()[0]
            if kind(op):
                cur.append(op)
    return out


def main():
    args = sys.argv[1:]
    name = KERNEL
    if args[:1] == ["--kernel"]:
        name, args = args[1], args[2:]
    text = assembly(args)
    lines = kernel_text(text, name)
    print(f"kernel {name}\nflags {' '.join(args) or '(none)'}\nresources {resources(text, name)}")
    for hdr, blocks in loops(lines).items():
        ops_all = [o for _, ops in blocks for o in ops]
        if not any(o.startswith("v_max3_f32") for o in ops_all):
            continue   # the node cache's fill loop
        box = next(ops for _, ops in blocks if name_block(ops) == "box")
        print(f"\nloop {hdr} ({'IEEE division' if any(o.startswith('v_div_scale') for o in box) else 'exact fast division'})")
        print(f"  {'block':10s} {'is':7s} {'VALU':>5s} {'SALU':>5s} {'VMEM':>5s} {'LDS':>4s}")
        total = {}
        for label, ops in blocks:
            c = {k: sum(kind(o) == k for o in ops) for k in ("valu", "salu", "vmem", "lds")}
            n = name_block(ops)
            for k, v in c.items():
                total[(n, k)] = total.get((n, k), 0) + v
            print(f"  {label:10s} {n:7s} {c['valu']:5d} {c['salu']:5d} {c['vmem']:5d} {c['lds']:4d}")
        print("  by name: " + ", ".join(f"{n} {total[(n, 'valu')]}v/{total[(n, 'salu')]}s"
                                         for n in OrderedDict((n, 0) for n, _ in total)))
        print(f"  whole loop body: {sum(kind(o) == 'valu' for o in ops_all)} VALU, {sum(kind(o) == 'salu' for o in ops_all)} SALU")


if __name__ == "__main__":
    main()
