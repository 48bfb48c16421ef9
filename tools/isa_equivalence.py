#!/usr/bin/env python3
"""Per-function device-code comparison of two builds of one HIP translation unit (gfx950).

usage: tools/isa_equivalence.py PARENT.o NEW.o
       tools/isa_equivalence.py UNIT.o          (lists the kernels of one object: a host-runtime unit must have none)

For every kernel of PARENT.o: its instructions (PC-relative address arithmetic after s_getpc_b64 masked; the s_nop padding between a function's
last instruction and the next symbol's alignment dropped -- it depends on which function the compiler places next, not on the function), its
kernel descriptor (64 bytes minus the code-entry offset) and its metadata (registers, LDS, scratch, kernarg size).  Kernels only NEW.o has are listed apart.  Then every
other function symbol of the code object -- the out-of-line device functions the kernels call through those masked addresses -- by its
instructions, normalised the same way; one that only PARENT.o or only NEW.o has counts as a difference.  Exit status 1 when a kernel of
PARENT.o differs or is missing, or a function differs.  Needs the ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-objdump,
llvm-readelf); runs on the host, no device.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp, tag):
    fat = os.path.join(tmp, tag + ".fatbin")
    tool("llvm-objcopy", "--dump-section=.hip_fatbin=" + fat, obj, os.path.join(tmp, tag + ".stripped"))
    target = [t for t in tool("clang-offload-bundler", "--list", "--type=o", "--input=" + fat).split() if "gfx950" in t][0]
    co = os.path.join(tmp, tag + ".co")
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + target, "--input=" + fat, "--output=" + co)
    return co


def functions(co):
    """symbol -> normalised instruction list"""
    out, cur = {}, None
    pcrel = 0
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            pcrel = 0
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()
        if not ins:
            continue
        if ins.startswith("s_getpc_b64"):
            pcrel = 2   # the next s_add_u32 / s_addc_u32 pair adds a PC-relative offset
        elif pcrel and (ins.startswith("s_add_u32") or ins.startswith("s_addc_u32")):
            ins = ins.rsplit(",", 1)[0] + ", <pcrel>"
            pcrel -= 1
        cur.append(ins)
    for body in out.values():   # alignment padding up to the next symbol ("...": zeros the disassembler elides)
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return out


def descriptors(co):
    """kernel -> 64-byte descriptor with the code-entry offset (bytes 16..23) zeroed"""
    data = open(co, "rb").read()
    secs = {}
    for line in tool("llvm-readelf", "-S", "-W", co).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for line in tool("llvm-readelf", "-s", "-W", co).splitlines():
        p = line.split()
        if len(p) >= 8 and p[-1].endswith(".kd"):
            addr = int(p[1], 16)
            va, off = secs[".rodata"]
            b = bytearray(data[off + addr - va: off + addr - va + 64])
            b[16:24] = bytes(8)
            out[p[-1][:-3]] = bytes(b)
    return out


def device_functions(co):
    """the FUNC symbols that are not kernels (no <name>.kd beside them)"""
    names, kds = set(), set()
    for line in tool("llvm-readelf", "-s", "-W", co).splitlines():
        p = line.split()
        if len(p) >= 8 and p[-1].endswith(".kd"):
            kds.add(p[-1][:-3])
        elif len(p) >= 8 and p[3] == "FUNC" and p[6] != "UND":
            names.add(p[-1])
    return names - kds


def metadata(co):
    """kernel -> sorted scalar metadata lines (.sgpr_count, .vgpr_count, LDS, scratch, ...)"""
    text = tool("llvm-readelf", "--notes", co)
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        keys = sorted(l.strip() for l in block.splitlines() if re.match(r"\s+\.(\w+):\s+\S", l) and ".name" not in l and ".symbol" not in l)
        out[name] = keys
    return out


def main():
    if len(sys.argv) == 2:
        with tempfile.TemporaryDirectory() as tmp:
            try:
                kernels = sorted(descriptors(code_object(sys.argv[1], tmp, "a")))
            except subprocess.CalledProcessError:   # no .hip_fatbin section: the unit has no device code at all
                kernels = []
        print("\n".join(kernels + ["%d kernel(s) in %s" % (len(kernels), os.path.basename(sys.argv[1]))]))
        return 0
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = code_object(sys.argv[1], tmp, "a"), code_object(sys.argv[2], tmp, "b")
        fa, fb = functions(a), functions(b)
        da, db = descriptors(a), descriptors(b)
        ma, mb = metadata(a), metadata(b)
        na, nb = device_functions(a), device_functions(b)
    bad = 0
    for k in sorted(da):
        what = []
        if k not in db:
            what.append("missing")
        else:
            if fa.get(k) != fb.get(k):
                what.append("instructions")
            if da[k] != db[k]:
                what.append("descriptor")
            if ma.get(k) != mb.get(k):
                what.append("metadata")
        bad += bool(what)
        print("%-8s %5d instructions  %s" % ("DIFFERS" if what else "same", len(fa.get(k, [])), k) + ("  (" + ", ".join(what) + ")" if what else ""))
    for k in sorted(set(db) - set(da)):
        print("new      %5d instructions  %s" % (len(fb.get(k, [])), k))
    badFn = 0
    for k in sorted(na | nb):
        what = "only in the parent" if k not in nb else "only in the new object" if k not in na else "instructions" if fa.get(k) != fb.get(k) else ""
        badFn += bool(what)
        print("%-8s %5d instructions  %s  [function]" % ("DIFFERS" if what else "same", len((fa if k in na else fb).get(k, [])), k) + ("  (" + what + ")" if what else ""))
    print("%d kernel(s) of the parent, %d differ; %d other function(s), %d differ" % (len(da), bad, len(na | nb), badFn))
    return 1 if bad or badFn else 0


if __name__ == "__main__":
    sys.exit(main())
