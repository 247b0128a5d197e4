#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libwm_hip.so, kernel by kernel (no GPU needed).

For a host-side refactor: the set of device functions and the bytes of each must not change.  Takes the .hip_fatbin
section out of each library, unbundles the gfx950 code object, and compares name, size and bytes of every function
symbol in .text.  Also compares the exported wm_* symbols.  Exit status 0 = identical.
For every function whose bytes differ, the register / scratch / LDS figures of the code object's metadata are printed for both sides.

usage: tools/device_code_diff.py <a.so> <b.so> [--allow-renamed SUBSTR ...] [--rename REGEX REPL ...]
  --allow-renamed: a function whose mangled name contains SUBSTR may be named differently in the two libraries
                   (it is matched by SUBSTR and its bytes are still compared)
  --rename:        re.sub(REGEX, REPL) is applied to the mangled names of <a.so> before matching (repeatable): pairs up template
                   instances whose argument list changed; every pairing is printed and the bytes are still compared
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else (shutil.which(name) or name)


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def device_functions(lib, tmp):
    """name -> bytes of every function symbol in .text of the library's gfx950 code object"""
    tag = os.path.join(tmp, os.path.basename(lib))
    run(tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, tag + ".fatbin")
    run(tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + tag + ".fatbin", "--output=" + tag + ".co")
    text_addr = text_off = None
    for line in run(tool("llvm-readelf"), "-S", "-W", tag + ".co").splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[1] == ".text":
            text_addr, text_off = int(f[3], 16), int(f[4], 16)
    if text_addr is None:
        sys.exit(f"{lib}: no .text in the gfx950 code object")
    blob = open(tag + ".co", "rb").read()
    out = {}
    for line in run(tool("llvm-objdump"), "-t", tag + ".co").splitlines():
        f = line.split()
        # address flags... F .text size [visibility] name
        if ".text" in f and "F" in f[1:f.index(".text")]:
            addr, size, name = int(f[0], 16), int(f[f.index(".text") + 1], 16), f[-1]
            out[name] = blob[text_off + addr - text_addr: text_off + addr - text_addr + size]
    if not out:
        sys.exit(f"{lib}: no function symbols found in the gfx950 code object")
    return out, resources(tag + ".co")


RES_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def resources(co):
    """kernel name -> {key: value} for RES_KEYS, from the amdhsa.kernels metadata note"""
    out = {}
    for block in re.split(r"\n  - \.", run(tool("llvm-readelf"), "--notes", co)):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(m.group(1)) for k in RES_KEYS for m in [re.search(r"\.?" + k + r":\s+(\d+)", block)] if m}
    return out


def exports(lib):
    return sorted(l.split()[-1] for l in run("nm", "-D", "--defined-only", lib).splitlines() if l.split()[-1].startswith("wm_"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--allow-renamed", nargs="*", default=[])
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a")), os.makedirs(os.path.join(tmp, "b"))
        (fa, ra), (fb, rb) = device_functions(args.a, os.path.join(tmp, "a")), device_functions(args.b, os.path.join(tmp, "b"))
    bad = 0
    for rx, repl in args.rename:
        for old in sorted(fa):
            new = re.sub(rx, repl, old)
            if new != old:
                if new in fa:
                    sys.exit(f"--rename {rx}: {old} -> {new} collides with another function of {args.a}")
                print(f"renamed: {old} -> {new}" + ("" if new in fb else "  (not in b)"))
                fa[new] = fa.pop(old)
                if old in ra:
                    ra[new] = ra.pop(old)
    for sub in args.allow_renamed:
        na, nb = [n for n in fa if sub in n], [n for n in fb if sub in n]
        if len(na) == 1 and len(nb) == 1 and na[0] != nb[0]:
            print(f"renamed (allowed): {na[0]} -> {nb[0]}")
            fb[na[0]] = fb.pop(nb[0])
    for n in sorted(set(fa) - set(fb)):
        print("only in a:", n); bad += 1
    for n in sorted(set(fb) - set(fa)):
        print("only in b:", n); bad += 1
    for n in sorted(set(fa) & set(fb)):
        if fa[n] != fb[n]:
            nd = sum(x != y for x, y in zip(fa[n], fb[n])) if len(fa[n]) == len(fb[n]) else -1
            print(f"differs: {n}  size {len(fa[n])} vs {len(fb[n])}" + (f", {nd} bytes differ" if nd >= 0 else "")); bad += 1
            if not (ra.get(n) and rb.get(n) and set(ra[n]) == set(rb[n]) == set(RES_KEYS)):
                print("    resources: not found in the metadata of both code objects")
            else:
                print("    resources " + ("EQUAL " if ra[n] == rb[n] else "DIFFER") + "  " +
                      "  ".join(f"{k} {ra[n].get(k)}" + ("" if ra[n].get(k) == rb[n].get(k) else f" -> {rb[n].get(k)}") for k in RES_KEYS))
    print(f"device functions: {len(fa)} vs {len(fb)}, {sum(len(v) for v in fa.values())} vs {sum(len(v) for v in fb.values())} bytes of code")
    ea, eb = exports(args.a), exports(args.b)
    for n in sorted(set(ea) ^ set(eb)):
        print("export only in", "a:" if n in ea else "b:", n); bad += 1
    print(f"exported wm_* symbols: {len(ea)} vs {len(eb)}")
    print("IDENTICAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
