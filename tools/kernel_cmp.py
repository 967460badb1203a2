#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same machine code?

    tools/kernel_cmp.py A B [object ...]

A, B: two object files, or two trees (then waveforms_amd/csrc/_obj/<object> of each, default every object that is
built with an offload arch: the `OBJ :=` line of waveforms_amd/csrc/Makefile but wfk_compile.o).  The code object is taken out of each object file as tools/kernel_regs.sh does, disassembled
with llvm-objdump -d, and compared per function symbol (kernels and the device functions they call): the encoded
instruction words (branches are PC-relative and a reference to another function is compared by what it reaches, so
a kernel that merely moved compares equal) and, for kernels, the metadata kernel_regs.sh prints (VGPR / AGPR / SGPR, spills,
LDS, scratch).  Exit status 0: same set of kernels, every one identical.
"""
import os
import re
import subprocess
import sys
import tempfile

B = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size", "private_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(obj):
    """{function symbol: (metadata tuple of a kernel or None, [encoded instruction words])}"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "k.co")
        if ".hip_fatbin" not in run(f"{B}/llvm-readelf", "-S", obj):
            return {}                                        # host code only (wfk_api.o today): no kernels
        run(f"{B}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj)
        run(f"{B}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
        notes = run(f"{B}/llvm-readelf", "--notes", co)
        dis = run(f"{B}/llvm-objdump", "-d", co)
    meta, cur = {}, {}
    for line in notes.splitlines() + ["  - .end:"]:
        m = re.match(r"  (-| ) \.(\w+):\s*(.*)", line)     # the keys of a kernel's record; its first one has the dash
        if not m:
            continue
        if m.group(1) == "-":
            if "name" in cur:
                meta[cur["name"]] = tuple(cur.get(x) for x in META)
            cur = {}
        cur[m.group(2)] = m.group(3).strip()
    # every function of the code object (kernels and the device functions they call): its address, its words.  A
    # reference from one function to another -- s_getpc_b64, then s_add_u32 with the 32-bit distance -- is recorded as
    # the function and offset it reaches: which functions come first in the object is not part of a kernel's code
    code, start, refs, sym, prev = {}, {}, [], None, ""
    for line in dis.splitlines():
        m = re.match(r"([0-9a-f]+) <(.+)>:$", line)
        if m:
            sym = m.group(2)
            code[sym], start[sym] = [], int(m.group(1), 16)
            continue
        m = re.search(r"^\s*(\S+).*// ([0-9A-F]+): ([0-9A-F ]+)$", line)
        if m and sym is not None:
            words = m.group(3).split()
            if m.group(1) == "s_add_u32" and prev == "s_getpc_b64" and len(words) == 2:
                dist = int(words[1], 16) - (1 << 32 if words[1][0] in "89ABCDEF" else 0)
                refs.append((sym, len(code[sym]) + 1, int(m.group(2), 16) + dist))
            code[sym].extend(words)
            prev = m.group(1)
    by_addr = sorted((a, k) for k, a in start.items())
    for sym, at, target in refs:
        a, k = max((x for x in by_addr if x[0] <= target), default=(0, None))
        if k is not None and target < a + 4 * len(code[k]):
            code[sym][at] = f"{k}+{target - a}"
    missing = [k for k in meta if k not in code]
    if missing:
        sys.exit(f"{obj}: no code found for {missing[:3]}")
    return {k: (meta.get(k), code[k]) for k in code}


def default_objects():
    """the objects of the Makefile's `OBJ :=` line, minus the one that is host code only"""
    makefile = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "waveforms_amd", "csrc", "Makefile")
    with open(makefile) as f:
        line = next(l for l in f if l.startswith("OBJ :="))
    return [os.path.basename(o) for o in line.split()[2:] if os.path.basename(o) != "wfk_compile.o"]


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = sys.argv[1:3]
    if os.path.isdir(a):
        names = sys.argv[3:] or default_objects()
        pairs = [(n, *(os.path.join(t, "waveforms_amd/csrc/_obj", n) for t in (a, b))) for n in names]
    else:
        pairs = [(os.path.basename(a), a, b)]
    bad = 0
    for label, oa, ob in pairs:
        ka, kb = kernels(oa), kernels(ob)
        only = sorted(set(ka) ^ set(kb))
        for k in only:
            print(f"{label}: only in {'A' if k in ka else 'B'}: {k}")
        same = 0
        for k in sorted(set(ka) & set(kb)):
            (ma, ca), (mb, cb) = ka[k], kb[k]
            if ma == mb and ca == cb:
                same += 1
                continue
            bad += 1
            name = run("c++filt", k).strip()
            print(f"{label}: DIFFERENT {name[:110]}")
            if ma != mb:
                print("    metadata " + "  ".join(f"{x} {p}->{q}" for x, p, q in zip(META, ma, mb) if p != q))
            if ca != cb:
                first = next((i for i, (p, q) in enumerate(zip(ca, cb)) if p != q), min(len(ca), len(cb)))
                print(f"    code {len(ca)} -> {len(cb)} words, first difference at word {first}")
        bad += len(only)
        words = sum(len(c) for _, c in ka.values())
        print(f"{label}: {len(ka)} functions in A, {len(kb)} in B, {same} identical "
              f"(instruction words and registers / spills / LDS / scratch), {words} instruction words in A")
    print("IDENTICAL" if not bad else f"{bad} DIFFERENCE(S)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
