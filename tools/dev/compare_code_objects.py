#!/usr/bin/env python3
"""Developer tool: are the kernels that existed before still the same instructions?

usage: compare_code_objects.py <libvfgs_hip.so of the parent build> <libvfgs_hip.so of this build>

`llvm-objdump -d --no-show-raw-insn` of every gfx950 code object inside both libraries, function by function, restricted to the functions
of the first library.  The literal of the s_add_u32 behind an s_getpc_b64 -- the distance to a symbol, which moves with the size of the
code object -- is left out of the comparison (and counted).  Prints the functions that differ with their first differing line, and the line
counts per code object that DESIGN.md quotes (4.5, 4.6, 4.8)."""
import re, struct, subprocess, sys, tempfile
from pathlib import Path

import shutil

OBJDUMP = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"


def code_objects(path):
    d = Path(path).read_bytes()
    out = []
    for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), d):
        b = m.start()
        (n,) = struct.unpack_from("<Q", d, b + 24)
        p = b + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", d, p)
            p += 24
            triple = d[p:p + tl].decode()
            p += tl
            if "gfx950" in triple and size:
                out.append(d[b + off:b + off + size])
    if not out and d[:4] == b"\x7fELF":
        out = [d]
    return out


NORM = [0]


def kernels(path, tmp):
    ks = {}
    for i, co in enumerate(code_objects(path)):
        f = Path(tmp) / f"co{i}.elf"
        f.write_bytes(co)
        text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", str(f)], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                cur = (i, m.group(1))
                ks[cur] = []
                continue
            if cur and line.strip():
                # instruction text without the address comment
                ins = re.sub(r"\s*//.*$", "", line).strip()
                # the distance from an s_getpc_b64 to a symbol (the constant-address operand behind it) depends on where the code object's
                # sections lie, not on the kernel: compared without the literal
                if ks[cur] and ks[cur][-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                    ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
                    NORM[0] += 1
                ks[cur].append(ins)
    return ks


with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
    a = kernels(sys.argv[1], t1)
    b = kernels(sys.argv[2], t2)
na = sum(len(v) for v in a.values())
same = diff = 0
lines = 0
for k, v in a.items():
    if k not in b:
        print("missing in new:", k)
        diff += 1
        continue
    if v == b[k]:
        same += 1
        lines += len(v)
    else:
        diff += 1
        print("DIFFERS:", k, len(v), len(b[k]))
        for x, y in zip(v, b[k]):
            if x != y:
                print("   ", x, "|", y)
                break
print("pc-relative literals normalised (both builds):", NORM[0])
new = [k for k in b if k not in a]
print(f"parent kernels/functions {len(a)} ({na} lines); identical {same} ({lines} lines); differing {diff}; new in this build {len(new)} ({sum(len(b[k]) for k in new)} lines)")
for i in sorted({k[0] for k in a}):
    print("code object", i, "parent lines", sum(len(v) for k, v in a.items() if k[0] == i), "this build, same kernels", sum(len(b[k]) for k in a if k[0] == i and k in b),
          "new kernels", len([k for k in new if k[0] == i]))
