"""The Rust shim (shim/rust/sampler_hip.rs) against include/mrt.h, without a Rust compiler.

`#[repr(C)]` makes rustc lay a struct out by the platform's C rules.  This test parses the shim's `#[repr(C)]`
declarations, applies those rules (natural alignment, fields in order, size rounded up to the alignment) and compares
every struct size and field offset with (a) what the C compiler reports for include/mrt.h (tests/native/layout.c) and
(b) the committed table shim/rust/layout.txt.  It also checks the shim's `extern "C"` block against the header and the
built library: every function exists, with the header's number of arguments.
"""
import os
import re
import subprocess

from conftest import ROOT

SHIM = os.path.join(ROOT, "shim", "rust", "sampler_hip.rs")
PRIM = {"u8": (1, 1), "i8": (1, 1), "u16": (2, 2), "i16": (2, 2), "u32": (4, 4), "i32": (4, 4), "f32": (4, 4),
        "u64": (8, 8), "i64": (8, 8), "f64": (8, 8), "usize": (8, 8)}


def _snake(name):
    return re.sub(r"(?<!^)(?=[A-Z])", "_", name).lower()


def _rust_structs():
    src = open(SHIM).read()
    out = {}
    for m in re.finditer(r"#\[repr\(C\)\](?:\s*#\[derive\([^)]*\)\])?\s*struct\s+(\w+)\s*\{(.*?)\}", src, re.S):
        name, body = m.group(1), m.group(2)
        fields, depth, cur = [], 0, ""
        for ch in body:                       # split on commas outside [..]
            if ch == "[":
                depth += 1
            if ch == "]":
                depth -= 1
            if ch == "," and depth == 0:
                fields.append(cur)
                cur = ""
            else:
                cur += ch
        fields.append(cur)
        out[name] = [tuple(s.strip() for s in f.split(":", 1)) for f in fields if ":" in f]
    return out


def _layout(structs):
    done = {}

    def size_align(ty):
        ty = ty.strip()
        if ty in PRIM:
            return PRIM[ty]
        if ty.startswith("*const") or ty.startswith("*mut"):
            return 8, 8
        m = re.fullmatch(r"\[\s*(.+?)\s*;\s*(\d+)\s*\]", ty)
        if m:
            s, a = size_align(m.group(1))
            return s * int(m.group(2)), a
        return one(ty)[:2]

    def one(name):
        if name in done:
            return done[name]
        off, align, fields = 0, 1, {}
        for fname, ty in structs[name]:
            s, a = size_align(ty)
            off = (off + a - 1) // a * a
            fields[fname] = (off, s)
            off += s
            align = max(align, a)
        size = (off + align - 1) // align * align
        done[name] = (size, align, fields)
        return done[name]

    return {n: one(n) for n in structs}


def _table(text):
    structs, fields = {}, {}
    for line in text.splitlines():
        p = line.split()
        if p and p[0] == "struct":
            structs[p[1]] = (int(p[2]), int(p[3]))
        elif p and p[0] == "field":
            s, f = p[1].split(".")
            fields[(s, f)] = (int(p[2]), int(p[3]))
    return structs, fields


def test_repr_c_structs_match_the_header_layout():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "layout"], stdout=subprocess.DEVNULL)
    live = subprocess.check_output([os.path.join(ROOT, "tests", "native", "layout")], text=True)
    committed = open(os.path.join(ROOT, "shim", "rust", "layout.txt")).read()
    assert live == committed, "include/mrt.h changed its layout: regenerate shim/rust/layout.txt and revisit sampler_hip.rs"
    c_structs, c_fields = _table(live)
    rust = _layout({k: v for k, v in _rust_structs().items() if v})
    need = {"mrt_camera", "mrt_frame", "mrt_rt", "mrt_texture", "mrt_material", "mrt_instance", "mrt_renderer", "mrt_light",
            "mrt_sky", "mrt_scene", "mrt_render_desc", "mrt_opts"}
    seen = set()
    for rname, (size, align, fields) in rust.items():
        cname = _snake(rname)
        if cname not in c_structs:
            continue
        seen.add(cname)
        assert (size, align) == c_structs[cname], (rname, size, align, c_structs[cname])
        c_names = [f for (s, f) in c_fields if s == cname]
        assert list(fields) == c_names, (rname, list(fields), c_names)          # same fields, same order
        for f, (off, sz) in fields.items():
            assert (off, sz) == c_fields[(cname, f)], (rname, f, (off, sz), c_fields[(cname, f)])
    assert need <= seen, need - seen


def test_extern_block_matches_header_and_library():
    from micro_raytracer_amd import _lib
    src = open(SHIM).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', src, re.S).group(1)
    hdr = open(os.path.join(ROOT, "include", "mrt.h")).read()
    L = _lib.lib()
    fns = re.findall(r"fn\s+(mrt_\w+)\s*\(([^)]*)\)", block)
    assert {"mrt_create", "mrt_destroy", "mrt_execute", "mrt_img", "mrt_last_error"} <= {n for n, _ in fns}
    for name, args in fns:
        assert hasattr(L, name), name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        c_args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        r_args = [a for a in args.split(",") if a.strip()]
        assert len(c_args) == len(r_args), (name, c_args, r_args)
    # the ABI version the shim passes is the library's
    assert re.search(r"abi_version:\s*(\d+)", src).group(1) == str(L.mrt_abi_version())


def test_feature_bit_names_match_the_kernel_header():
    """The F_* constants of micro_raytracer_amd/_abi.py are the enum of csrc/mrt_scene.h: same names, same values."""
    from micro_raytracer_amd import _abi
    src = open(os.path.join(ROOT, "micro_raytracer_amd", "csrc", "mrt_scene.h")).read()
    body = re.search(r"enum\s*:\s*u32\s*\{(\s*F_BOX\b.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    header = {name: int(value) for name, value in re.findall(r"\b(F_[A-Z]+)\s*=\s*(\d+)u\b", body)}
    python = {name: getattr(_abi, name) for name in dir(_abi) if re.fullmatch(r"F_[A-Z]+", name)}
    assert len(header) == 12 and header == python, (header, python)
