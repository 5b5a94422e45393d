#!/usr/bin/env python3
"""Compare the device assembly of two builds, kernel by kernel: asm_compare.py OLD_DIR NEW_DIR

Each directory holds NAME.s files (hipcc -S --cuda-device-only with the Makefile's FLAGS, one per kernel source).  Per kernel,
paired by demangled name: the instruction lines (comments and directives dropped, .LBB<n>_ without the function index), the
.amdhsa_ block and the kernel's metadata entry (.args, register, spill, scratch and LDS figures; not its two name fields).
Kernels that were renamed pair through RENAMES.  Prints one line per source and every kernel that differs; exit status 1 if any."""
import re, subprocess, sys
from pathlib import Path

RENAMES = [(r"pt_megakernel_list<(.*)>$", r"pt_megakernel<\1, mrt::TileList>"), (r"dn_pass_env$", "dn_pass<true>"), (r"dn_pass$", "dn_pass<false>")]


def kernels(path):
    text = path.read_text()
    code, _, meta = text.partition("\n\t.amdgpu_metadata\n")
    out, sym, part = {}, None, None
    for line in code.split("\n"):
        m = re.match(r"\t\.type\t(\S+),@function", line)
        if m:
            sym, part = m.group(1), out.setdefault(m.group(1), {"insn": [], "hsa": [], "meta": []})
        elif sym and line.startswith(".Lfunc_end"):
            sym = None
        elif sym:
            body = line.split(";")[0].strip()
            if body.startswith(".amdhsa_"):
                part["hsa"].append(re.sub(r"^\.amdhsa_kernel \S+", ".amdhsa_kernel", body))
            elif body and not body.startswith(".") or re.match(r"\.LBB\d+_\d+:", body):
                part["insn"].append(re.sub(r"\.LBB\d+_", ".LBB_", body).replace(sym, "<self>"))
    for entry in re.split(r"\n  - (?=\.agpr_count)", meta.partition("\namdhsa.target:")[0])[1:]:
        name = re.search(r"\n    \.name: +(\S+)", entry).group(1)
        out[name]["meta"] = [ln for ln in entry.split("\n") if not re.match(r"    \.(name|symbol):", ln)]
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for sym, name in zip(out, names):
        name = re.sub(r"^void ", "", name.split("(")[0])
        for pat, to in RENAMES:
            name = re.sub(pat, to, name)
        res[name] = out[sym]
    return res


old_dir, new_dir = Path(sys.argv[1]), Path(sys.argv[2])
total = same = 0
for old_s in sorted(old_dir.glob("*.s")):
    a, b = kernels(old_s), kernels(new_dir / old_s.name)
    bad = sorted(set(a) ^ set(b)) + [k for k in a if k in b and a[k] != b[k]]
    for k in bad:
        parts = [p for p in ("insn", "hsa", "meta") if k in a and k in b and a[k][p] != b[k][p]]
        print(f"  DIFFERS {old_s.name} {k}: {', '.join(parts) or 'in one build only'}")
    n_kern = sum(1 for k in a if a[k]["hsa"])
    print(f"{old_s.name}: {len(a)} functions ({n_kern} kernels) compared, {len(a) - sum(1 for k in bad if k in a)} identical")
    total += len(a)
    same += len(a) - sum(1 for k in bad if k in a)
print(f"{total} compared, {same} identical")
sys.exit(0 if total == same and total else 1)
