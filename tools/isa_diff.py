#!/usr/bin/env python3
"""tools/isa_diff.py <dir A> <dir B>: compare, kernel by kernel, the gfx950 assembly of two builds of the csrc sources
(directories of *-hip-amdgcn-amd-amdhsa-gfx950.s files as tools/isa.sh / -save-temps=obj leave them).  Prints the kernels whose
instruction stream differs, the kernels only one side has, and per new kernel its register / spill numbers."""
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
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt):
        res[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    return res


a_dir, b_dir = sys.argv[1], sys.argv[2]
same = diff = 0
for fa in sorted(glob.glob(os.path.join(a_dir, "*gfx950.s"))):
    fb = os.path.join(b_dir, os.path.basename(fa))
    ka, kb = kernels(fa), kernels(fb)
    mb = meta(fb)
    for k in sorted(ka):
        if k not in kb:
            print(f"ONLY IN A  {k}")
        elif ka[k] == kb[k]:
            same += 1
        else:
            diff += 1
            print(f"DIFFERS    {k}  ({len(ka[k])} -> {len(kb[k])} instructions)")
    for k in sorted(set(kb) - set(ka)):
        n = len(kb[k])
        nexp = sum(t.startswith(("v_exp_f32", "v_rcp_f32")) for t in kb[k])
        npk = sum(t.startswith("v_pk_") for t in kb[k])
        print(f"NEW        {k}  {n} instructions ({npk} packed, {nexp} v_exp/v_rcp)  sgpr/vgpr/spill {mb.get(k)}")
print(f"{same} kernels identical, {diff} differ")
