#!/usr/bin/env python3
"""Host-only refactors must leave the device code alone: disassembles every gfx950 code object of two builds of
libneo_planner_hip.so (llvm-objdump -d on the entries of the library's offload bundles; no GPU needed) and compares
the instructions symbol by symbol: mnemonics, operands and encodings.  The address a listing line carries is left out --
where a kernel sits in its code object follows the order in which the unit instantiates its templates, and branch targets
are printed relative to their symbol; so is the padding behind the last kernel of a code object, and so is the literal of
the s_add_u32 behind an s_getpc_b64 (the distance to a table elsewhere in the code object: it moves when a kernel leaves
the unit).

    python tools/compare_device_code.py old.so [new.so]      (default new = the in-tree build)
"""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(lib):
    """{symbol: [instruction lines]} over all gfx950 code objects of `lib`"""
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/llvm/bin/llvm-objdump"
    data = open(lib, "rb").read()
    syms = {}
    for m in re.finditer(MAGIC, data):  # one uncompressed bundle per translation unit: magic, count, (offset, size, triple)*
        p = m.start()
        q = p + len(MAGIC) + 8
        for _ in range(struct.unpack_from("<Q", data, p + len(MAGIC))[0]):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" not in triple:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(data[p + off:p + off + size]); f.flush()
                dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                s = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if s:
                    cur = s.group(1)
                    assert cur not in syms, cur
                    syms[cur] = []
                elif cur:
                    syms[cur].append(re.sub(r"// [0-9A-F]{12}: ", "// ", line))
    for lines in syms.values():
        # s_getpc_b64 / s_add_u32 lo, lo, literal / s_addc_u32 hi, hi, ...: the distance from here to a table or function
        # elsewhere in the code object -- layout, as the addresses are.  Only this exact triple is masked.
        for i in range(1, len(lines) - 1):
            if ("s_getpc_b64" in lines[i - 1] and re.match(r"\s*s_add_u32 s\d+, s\d+, 0x[0-9a-f]+\s", lines[i])
                    and re.match(r"\s*s_addc_u32 s\d+, s\d+, ", lines[i + 1])):
                lines[i] = re.sub(r"0x[0-9a-f]+(\s+// [0-9A-F]{8}) [0-9A-F]{8}", r"<pcrel>\1", lines[i])
    for lines in syms.values():  # (the zero padding objdump prints as "..." behind a code object's last kernel)
        while lines and lines[-1].strip() in ("", "..."):
            lines.pop()
    return syms


def main():
    old = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "neo-planner_amd", "neo_planner_amd", "libneo_planner_hip.so")
    a, b = kernels(old), kernels(new)
    bad = sorted(set(a) ^ set(b)) + sorted(k for k in a if k in b and a[k] != b[k])
    for k in bad:
        print("DIFF", k, "(only in one library)" if (k in a) != (k in b) else "")
    print(f"{len(a)} / {len(b)} symbols, {sum(map(len, a.values()))} instruction lines: {len(bad)} symbols differ")
    sys.exit(1 if bad or not a else 0)


if __name__ == "__main__":
    main()
