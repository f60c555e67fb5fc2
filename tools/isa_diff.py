#!/usr/bin/env python3
"""tools/isa_diff.py <dir A> <dir B>: compare, kernel by kernel, the gfx950 assembly of two builds of the csrc sources
(directories of *-hip-amdgcn-amd-amdhsa-gfx950.s files as tools/isa.sh / -save-temps=obj leave them).  Prints the kernels whose
instruction stream differs (with instructions, sgpr / vgpr / spilled vgpr / scratch bytes of both sides), the kernels only one
side has, and per new kernel the same numbers.  The kernels of all files of a directory are pooled, so a kernel that moved from one
source file to another is compared with itself.
--ignore-params: match template kernels by name and template arguments alone, so that a kernel whose PARAMETER LIST changed (a
mangled name with another tail) is still compared with its predecessor instead of showing up as one removed and one new."""
import glob
import os
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = line.split(";")[0].strip()   # comments carry source-independent noise only
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)   # block labels carry the function's ordinal in its file
        if t and not t.startswith("."):
            body.append(t)
    return out


def meta(path):
    txt = open(path).read()
    res = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt):
        res[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(2)))   # sgpr, vgpr, spilled vgpr, scratch bytes
    return res


args = [a for a in sys.argv[1:] if a != "--ignore-params"]
IGNORE_PARAMS = len(args) != len(sys.argv) - 1
a_dir, b_dir = args[0], args[1]


def key(name):
    # _Z<name>I<template args>E E v <parameters>: a templated kernel returns void, so its parameters start behind the last "EEv"
    i = name.rfind("EEv")
    return name[:i + 2] if IGNORE_PARAMS and i > 0 else name


def offsets_only(a, b):
    """The same instructions except for the immediate offset of scalar loads from the kernel-argument segment: what a grown
    parameter list does to a kernel that does not use the new parameter."""
    if len(a) != len(b):
        return False
    strip = lambda t: re.sub(r"(s_load_dword\w*\s+s\S+\s+s\[\d+:\d+\],)\s*\S+$", r"\1", t)
    return all(x == y or (x.startswith("s_load_dword") and strip(x) == strip(y)) for x, y in zip(a, b))


def pool(d):
    k, m = {}, {}
    for f in sorted(glob.glob(os.path.join(d, "*gfx950.s"))):
        k.update({key(n): v for n, v in kernels(f).items()})
        m.update({key(n): v for n, v in meta(f).items()})
    return k, m


same = diff = moved = 0
(ka, ma), (kb, mb) = pool(a_dir), pool(b_dir)
for k in sorted(ka):
    if k not in kb:
        print(f"ONLY IN A  {k}")
    elif ka[k] == kb[k]:
        same += 1
    elif offsets_only(ka[k], kb[k]):
        moved += 1
        print(f"ARG OFFSET {k}  ({len(ka[k])} instructions; only the offsets of kernel-argument loads differ)")
    else:
        diff += 1
        print(f"DIFFERS    {k}  ({len(ka[k])} -> {len(kb[k])} instructions)  sgpr/vgpr/spill/scratch {ma.get(k)} -> {mb.get(k)}")
for k in sorted(set(kb) - set(ka)):
    n = len(kb[k])
    nexp = sum(t.startswith(("v_exp_f32", "v_rcp_f32")) for t in kb[k])
    npk = sum(t.startswith("v_pk_") for t in kb[k])
    print(f"NEW        {k}  {n} instructions ({npk} packed, {nexp} v_exp/v_rcp)  sgpr/vgpr/spill/scratch {mb.get(k)}")
print(f"{same} kernels identical, {moved} with moved kernel-argument offsets only, {diff} differ")
