#!/usr/bin/env python3
"""isa_compare.py <old.o>[,<old2.o>...] <new.o>[,<new2.o>...] <name-part> [<name-part> ...]: are the gfx950 kernels whose
mangled names contain one of the parts the same in two HIP objects?  Either side may be a comma-separated list of objects,
whose kernels are merged by mangled name (a kernel that has moved to another file is found wherever it lives now).
Compares each kernel's instructions (addresses, branch targets and the fill behind the last instruction stripped) and its
metadata note (registers, LDS, scratch), lists the kernels only one object has, and prints registers / LDS / scratch of
every kernel it looked at.  Exit status 1 if a kernel that both objects have differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def device_code(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", f"--input={fat}", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    return dis, notes


def kernels(dis, parts):
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1) if any(p in m.group(1) for p in parts) else None
            if name:
                out[name] = []
            continue
        if name and line.strip():
            text = re.sub(r"^\s*[0-9a-f]+:\s*", "", line)                 # address
            text = re.sub(r"//.*$", "", text)                              # objdump's address comments
            text = re.sub(r"<[^>]+>", "<L>", text)                         # branch targets by symbol + offset
            out[name].append(re.sub(r"\s+", " ", text).strip())
    # what follows a kernel's last instruction up to the next symbol is the assembler's alignment fill, or the padding behind the
    # last kernel of the section: it depends on the kernel's neighbours in the file, not on the kernel
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."):
            body.pop()
    return out


def metadata(notes, parts):
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m or not any(p in m.group(1) for p in parts):
            continue
        keep = {}
        for key in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
                    "sgpr_spill_count", "max_flat_workgroup_size", "kernarg_segment_size", "wavefront_size"):
            k = re.search(r"\." + key + r":\s+(\S+)", blk)
            keep[key] = k.group(1) if k else None
        out[m.group(1)] = keep
    return out


def main():
    old, new, parts = sys.argv[1].split(","), sys.argv[2].split(","), sys.argv[3:]
    (k0, m0), (k1, m1) = ({}, {}), ({}, {})
    with tempfile.TemporaryDirectory() as tmp:
        for objs, tag, k, m in ((old, "old", k0, m0), (new, "new", k1, m1)):
            for q, obj in enumerate(objs):
                dis, notes = device_code(obj, tmp, f"{tag}{q}")
                k.update(kernels(dis, parts))
                m.update(metadata(notes, parts))
    bad = 0
    for name in sorted(set(k0) | set(k1)):
        m = m1.get(name) or m0.get(name) or {}
        res = (f"vgpr {m.get('vgpr_count')} sgpr {m.get('sgpr_count')} lds {m.get('group_segment_fixed_size')} "
               f"scratch {m.get('private_segment_fixed_size')} spills {m.get('vgpr_spill_count')}")
        if name not in k0:
            print(f"NEW      {name}: {len(k1[name])} instructions, {res}")
        elif name not in k1:
            print(f"GONE     {name}")
        elif k0[name] == k1[name] and m0.get(name) == m1.get(name):
            print(f"SAME     {name}: {len(k1[name])} instructions, {res}")
        else:
            bad += 1
            print(f"DIFFERS  {name}: {len(k0[name])} -> {len(k1[name])} instructions, metadata {m0.get(name)} -> {m1.get(name)}")
    print(f"{len(set(k0) & set(k1))} kernels in both, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
