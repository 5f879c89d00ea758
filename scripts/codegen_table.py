#!/usr/bin/env python3
"""Per-kernel code generation of the four-lane rollout, pack and transpose kernels, before and after a change (no GPU).

Usage: codegen_table.py BEFORE_DIR AFTER_DIR [--old-batch-order] > profiles/rollout_body_codegen.json
Each directory holds srbd_kernels.s and srbd_batch.s, made with
    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/FILE.hip -o DIR/FILE.s
For every instantiation: VGPRs, SGPRs, scratch bytes, static LDS bytes, instruction count and whether the instruction
text is the same in both (labels, symbol names and comments aside).  Kernels are matched by their demangled name;
--old-batch-order reads BEFORE's batch_rollout_kernel<KIND, HT, ST, EXT, CEMT, ENVT> as <KIND, HT, ST, CEMT, EXT, ENVT>.
"""
import hashlib
import json
import re
import subprocess
import sys

FAMILIES = r"(rollout_quad_kernel|rollout_ga_quad_kernel|batch_rollout_kernel|batch_rollout_ga_kernel|batch_pack\w*kernel|\btranspose_kernel|batch_transpose_kernel)"


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path, swap):
    asm = open(path).read()
    names = [m.group(1) for m in re.finditer(r"^(_Z\S+):", asm, re.M)]
    dem = demangle(names)
    res = {}
    for name in names:
        d = dem[name]
        if not re.search(FAMILIES, d.split("(")[0]):
            continue
        key = re.sub(r"^void srbd::", "", d.split("(")[0])
        key = key.replace("(srbd_kind)", "")
        if swap and key.startswith("batch_rollout_kernel<"):
            a = key[len("batch_rollout_kernel<"):-1].split(", ")
            a[3], a[4] = a[4], a[3]
            key = "batch_rollout_kernel<" + ", ".join(a) + ">"
        start = asm.index("\n" + name + ":") + len(name) + 2
        body = asm[start:asm.index(".Lfunc_end", start)].split("\n")
        text = []
        for l in body:
            l = l.split(";")[0].strip()
            if not l or l.startswith(".") or l.endswith(":"):
                continue
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            l = re.sub(r"_Z\w+", "SYM", l)
            text.append(l)
        meta = {k: int(v) for k, v in re.findall(r"\.set " + re.escape(name) + r"\.(num_vgpr|numbered_sgpr|private_seg_size), (\d+)", asm)}
        lds = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", asm)
        res[key] = {"num_vgpr": meta.get("num_vgpr"), "numbered_sgpr": meta.get("numbered_sgpr"),
                    "private_seg_size": meta.get("private_seg_size"), "lds_bytes": int(lds.group(1)) if lds else None,
                    "insts": len(text), "_hash": hashlib.sha1("\n".join(text).encode()).hexdigest()}
    return res


def main():
    before_dir, after_dir = sys.argv[1], sys.argv[2]
    swap = "--old-batch-order" in sys.argv
    rows = {}
    for f in ("srbd_kernels.s", "srbd_batch.s"):
        b = kernels(f"{before_dir}/{f}", swap)
        a = kernels(f"{after_dir}/{f}", False)
        for key in sorted(set(a) | set(b)):
            rb, ra = b.get(key), a.get(key)
            same = bool(rb and ra and rb.pop("_hash") == ra.pop("_hash"))
            for r in (rb, ra):
                if r:
                    r.pop("_hash", None)
            rows[key] = {"same_text": same, "before": rb, "after": ra}
    json.dump(rows, sys.stdout, indent=1)
    print()
    diff = [k for k, r in rows.items() if not r["same_text"]]
    print(f"{len(rows)} kernels, {len(rows) - len(diff)} with the same instruction text; differing:", file=sys.stderr)
    for k in diff:
        r = rows[k]
        print("  ", k, {x: (r["before"] or {}).get(x) for x in ("num_vgpr", "private_seg_size", "insts")}, "->",
              {x: (r["after"] or {}).get(x) for x in ("num_vgpr", "private_seg_size", "insts")}, file=sys.stderr)


if __name__ == "__main__":
    main()
