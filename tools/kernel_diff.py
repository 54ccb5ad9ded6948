r"""Compare the device code of two builds kernel by kernel.

usage: python tools/kernel_diff.py [--rename-b REGEX REPL] A B [hipcc flags...]

A and B are each a source tree (its path-tracer_amd/csrc/hip/*.hip are
compiled device-only for the offload architecture, with the flags of this
repository's build.py plus the flags given) or a directory of device code
objects (*.o, as `hipcc --cuda-device-only --no-gpu-bundle-output -c` writes
them).  Per side, every object is disassembled with llvm-objdump -d; addresses,
encodings, trailing comments and the alignment fill after a function's last
instruction are stripped and each kernel's body is hashed under its mangled
name; its register, LDS and scratch use and workgroup size
are read from the code object's metadata note.

Prints the kernels of each side by family, then the kernels present on one
side only, the kernels defined more than once on a side, and the kernels whose
body or metadata differ.  Exit status 1 if any of those lists is not empty.
The tool compares; it does not look for any instruction or pattern.

--rename-b: B's kernel names pass through re.sub(REGEX, REPL) before the two
sides are paired -- for a change that adds a template parameter, so that the
instantiations without the new flag meet their parent's (a trailing bool:
--rename-b '^(_ZN3ptd13extend_kernel.*)Lb0E(EEvNS_6dscene)' '\1\2' pairs
extend_kernel<..., false> with the parent's extend_kernel<...>).
"""
from __future__ import annotations

import concurrent.futures
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
import time
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("pt_build", ROOT / "path-tracer_amd" / "build.py")
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)

LLVM = Path(build.ROCM) / "lib" / "llvm" / "bin"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size", ".uses_dynamic_stack",
        ".max_flat_workgroup_size", ".kernarg_segment_size")
PADDING = ("", "...", "s_nop 0", "s_code_end")


def compile_tree(tree: Path, tmp: Path, extra):
    """Device-only objects of the tree's HIP sources -> [(source name, object, seconds)]."""
    srcs = sorted((tree / "path-tracer_amd" / "csrc" / "hip").glob("*.hip"))
    if not srcs:
        sys.exit(f"{tree}: no HIP sources and no objects")

    def one(src):
        obj = tmp / (src.stem + ".o")
        t = time.time()
        subprocess.run([build.HIPCC, *build.hip_flags(extra), "--cuda-device-only", "--no-gpu-bundle-output",
                        "-c", str(src), "-o", str(obj)], check=True)
        return src.name, obj, time.time() - t

    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1, 16)) as ex:
        return list(ex.map(one, srcs))


def bodies(obj: Path):
    """{symbol: sha256 of its instructions} of one code object."""
    text = subprocess.run([LLVM / "llvm-objdump", "-d", str(obj)], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.startswith("\t"):
            out[name].append(line.split("//")[0].strip())
    for body in out.values():
        # The fill between one function's end and the next one's aligned start
        # (or the section's end) is not the function's.
        while body and body[-1] in PADDING:
            body.pop()
    return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in out.items()}


def metadata(obj: Path):
    """{kernel name: {field: value}} from the code object's metadata note."""
    text = subprocess.run([LLVM / "llvm-readelf", "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("  - ."):          # a new entry of amdhsa.kernels
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.\w+): +(\S.*)$", line)
        if cur is not None and m:
            if m.group(1) == ".name":
                out[m.group(2)] = cur
            elif m.group(1) in META:
                cur[m.group(1)] = m.group(2)
        elif not line.startswith("    "):
            cur = None
    return out


def side(path: Path, tmp: Path, extra):
    """-> ({kernel: (body hash, metadata)}, [kernels defined twice], report lines)."""
    objs = sorted(path.glob("*.o"))
    objs = [(o.name, o, None) for o in objs] if objs else compile_tree(path, tmp, extra)
    kernels, twice, lines = {}, [], []
    for name, obj, secs in objs:
        body, meta = bodies(obj), metadata(obj)
        for k, md in meta.items():
            if k in kernels:
                twice.append(k)
            kernels[k] = (body.get(k), md)
        fam = Counter(family(k) for k in meta)
        lines.append(f"  {name}: {len(meta)} kernels" + (f", device pass {secs:.0f} s" if secs is not None else "") +
                     "".join(f"\n      {n:3d} {f}" for f, n in sorted(fam.items())))
    return kernels, twice, lines


def family(mangled: str) -> str:
    m = re.match(r"^_ZN\d+[a-z_]+?(\d+)", mangled)     # _ZN<len><namespace><len><name>...
    if not m:
        m = re.match(r"^_Z(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    return mangled[m.end():m.end() + n]


def main():
    rename = None
    if len(sys.argv) > 3 and sys.argv[1] == "--rename-b":
        rename = (re.compile(sys.argv[2]), sys.argv[3])
        del sys.argv[1:4]
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b, extra = Path(sys.argv[1]), Path(sys.argv[2]), sys.argv[3:]
    with tempfile.TemporaryDirectory(prefix="kernel_diff_a_") as ta, tempfile.TemporaryDirectory(prefix="kernel_diff_b_") as tb:
        ka, twice_a, la = side(a, Path(ta), extra)
        kb, twice_b, lb = side(b, Path(tb), extra)
    if rename:
        renamed = {}
        for k, v in kb.items():
            n = rename[0].sub(rename[1], k)
            if n in renamed:
                twice_b.append(n)
            renamed[n] = v
        kb = renamed
    print(f"A = {a}: {len(ka)} kernels\n" + "\n".join(la))
    print(f"B = {b}: {len(kb)} kernels\n" + "\n".join(lb))
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    differ = []
    for k in sorted(set(ka) & set(kb)):
        (ha, ma), (hb, mb) = ka[k], kb[k]
        if ha is None or ha != hb:
            differ.append(f"{k}: body")
        if ma != mb:
            differ.append(f"{k}: metadata " + ", ".join(f"{f} {ma.get(f)} -> {mb.get(f)}" for f in META if ma.get(f) != mb.get(f)))
    for title, items in (("only in A", only_a), ("only in B", only_b), ("defined twice in A", twice_a),
                         ("defined twice in B", twice_b), ("body or metadata differ", differ)):
        print(f"{title}: {len(items)}")
        for i in items:
            print("  " + i)
    same = len(set(ka) & set(kb)) - len({d.split(":")[0] for d in differ})
    print(f"identical in body and metadata: {same}")
    return 1 if only_a or only_b or twice_a or twice_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
