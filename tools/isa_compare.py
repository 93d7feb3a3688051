#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of the device units, kernel by kernel.

    python tools/isa_compare.py OLD_LIB_DIR NEW_LIB_DIR [--report FILE]

OLD_LIB_DIR / NEW_LIB_DIR hold the units' object files (chromosome3d_amd/_lib/*.o of two checkouts).  For every unit of the OLD
build that has device code (the host units' objects have no .hip_fatbin section and are skipped), the device code object is taken out of the object's .hip_fatbin section and, for every kernel of the OLD build, three things are compared with the NEW build:
the symbol exists, its instruction list (llvm-objdump, without addresses and raw bytes; branch targets as offsets from the kernel's
start) is the same, and its resource metadata (VGPRs, AGPRs, SGPRs, LDS, scratch, spills, wavefront size) is the same.  Kernels
only the NEW build has are listed as added.  Exit status 0 when nothing of the OLD build changed.
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".vgpr_spill_count", ".sgpr_spill_count", ".wavefront_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else name


def has_device_code(obj):
    out = subprocess.run([tool("llvm-readelf"), "-S", obj], check=True, capture_output=True, text=True).stdout
    return ".hip_fatbin" in out


def code_object(obj, tmp):
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    out = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([tool("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, obj, os.path.join(tmp, "discard.o")], check=True)
    subprocess.run([tool("clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + out,
                    "--unbundle"], check=True)
    return out


def kernels(co):
    """{symbol: [instructions]} of every function in the code object's text, branch targets made relative"""
    txt = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
                         capture_output=True, text=True).stdout
    funcs, cur, name = {}, None, None
    for line in txt.splitlines():
        m = re.match(r"^([0-9a-f]+)?\s*<(.+)>:$", line.strip()) if line.strip().endswith(">:") else None
        if m:
            name = m.group(2)
            cur = funcs.setdefault(name, [])
            continue
        if cur is None or not line.strip() or line.startswith("Disassembly"):
            continue
        ins = line.strip()
        ins = re.sub(r"//.*$", "", ins).strip()                       # the disassembler's address comments
        ins = re.sub(r"<" + re.escape(name) + r"\+0x([0-9a-f]+)>", r"<+0x\1>", ins)
        ins = re.sub(r"\b0x[0-9a-f]{8,}\b(?= <)", "", ins)             # absolute branch addresses (the relative form stays)
        if ins and ins != "...":                                        # ("...": the padding between functions)
            cur.append(ins)
    # the assembler pads the end of the text section with s_nop (the instruction prefetch may run past the last s_endpgm): that padding is
    # listed under whichever kernel comes last in the unit, and moves when a kernel is added behind it
    for body in funcs.values():
        while len(body) > 1 and body[-1] == "s_nop 0":
            body.pop()
    return funcs


def metadata(co):
    """{kernel symbol: {key: value}} from the code object's amdhsa metadata note (one "  - ." entry per kernel)"""
    txt = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    meta, cur = {}, None

    def close():
        if cur is not None and ".symbol" in cur:
            sym = cur.pop(".symbol")
            meta[sym[:-3] if sym.endswith(".kd") else sym] = cur

    for line in txt.splitlines():
        if re.match(r"^  - \.", line):          # a kernel's entry begins (its argument list is indented deeper)
            close()
            cur = {}
        if cur is None:
            continue
        s = line.strip().lstrip("- ").strip()
        for k in META_KEYS + (".symbol",):
            if s.startswith(k + ":"):
                cur[k] = s.split(":", 1)[1].strip()
    close()
    return meta


def demangle(names):
    if not names:
        return {}
    try:
        out = subprocess.run([tool("llvm-cxxfilt")], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    except FileNotFoundError:
        try:
            out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        except FileNotFoundError:
            out = []
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--report")
    a = ap.parse_args()
    lines, bad = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        for old in sorted(glob.glob(os.path.join(a.old, "*.o"))):
            unit = os.path.basename(old)
            new = os.path.join(a.new, unit)
            if not has_device_code(old):
                continue
            if not os.path.exists(new):
                lines.append("%s: missing in the new build" % unit); bad += 1
                continue
            od, nd = os.path.join(tmp, "old"), os.path.join(tmp, "new")
            os.makedirs(od, exist_ok=True); os.makedirs(nd, exist_ok=True)
            oco, nco = code_object(old, od), code_object(new, nd)
            ok, nk = kernels(oco), kernels(nco)
            om, nm = metadata(oco), metadata(nco)
            dm = demangle(sorted(set(om) | set(nm)))
            same = changed = 0
            for sym in sorted(om):
                if sym not in nm or sym not in nk:
                    lines.append("%s: %s: missing" % (unit, dm.get(sym, sym))); bad += 1; changed += 1
                elif ok.get(sym) != nk.get(sym):
                    lines.append("%s: %s: instructions differ (%d -> %d)" % (unit, dm.get(sym, sym), len(ok.get(sym, [])), len(nk[sym])))
                    bad += 1; changed += 1
                elif om[sym] != nm[sym]:
                    lines.append("%s: %s: metadata differ %s -> %s" % (unit, dm.get(sym, sym), json.dumps(om[sym]), json.dumps(nm[sym])))
                    bad += 1; changed += 1
                else:
                    same += 1
            added = sorted(set(nm) - set(om))
            lines.append("%s: %d kernels identical, %d changed, %d added" % (unit, same, changed, len(added)))
            for sym in added:
                md = nm[sym]
                lines.append("    + %s  vgpr %s agpr %s sgpr %s lds %s scratch %s spills %s/%s" % (
                    dm.get(sym, sym), md.get(".vgpr_count"), md.get(".agpr_count"), md.get(".sgpr_count"),
                    md.get(".group_segment_fixed_size"), md.get(".private_segment_fixed_size"), md.get(".vgpr_spill_count"),
                    md.get(".sgpr_spill_count")))
    lines.append("RESULT: %s" % ("no existing kernel changed" if bad == 0 else "%d differences" % bad))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.report:
        with open(a.report, "w") as f:
            f.write(text)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
