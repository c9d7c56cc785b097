#!/usr/bin/env python3
"""VGPR / SGPR / scratch / LDS of the gfx950 kernels in objects of libislands_amd.so:
    python tools/kernel_resources.py islands_amd/lib/obj/search.o [name-filter]
    python tools/kernel_resources.py --hash islands_amd/lib/obj/search*.o
--hash adds a fingerprint of each kernel's machine code (sha256 over its disassembly without
addresses), so that two builds can be compared kernel by kernel with `diff`.  An argument that is
not a file is the name filter."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def code_hashes(code_object):
    """symbol -> sha256 of its instructions (`llvm-objdump -d --no-show-raw-insn`, split at the
    `<symbol>:` lines, the trailing `// address` comments stripped; a `...` of zeros that ends a symbol is left
    out: it is the alignment padding up to the next symbol and depends on what follows the kernel in the object)"""
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", code_object], capture_output=True,
                         text=True, check=True).stdout
    out, cur, pad = {}, None, False
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur, pad = out.setdefault(m.group(1), hashlib.sha256()), False  # (a `...` held back was padding)
        elif cur is not None and line.strip() == "...":
            pad = True
        elif cur is not None and line.strip():
            if pad:  # zeros inside the symbol's body are code like any other
                cur.update(b"...\n")
                pad = False
            cur.update(re.sub(r"\s*//.*$", "", line).strip().encode() + b"\n")
    return {k: v.hexdigest()[:16] for k, v in out.items()}


def main():
    args = [a for a in sys.argv[1:] if a != "--hash"]
    want_hash = len(args) != len(sys.argv) - 1
    objs = [a for a in args if os.path.isfile(a)]
    flt = next((a for a in args if not os.path.isfile(a)), "")
    if not objs:
        sys.exit(__doc__)
    for obj in objs:
        sections = subprocess.run(["objdump", "-h", obj], capture_output=True, text=True, check=True).stdout
        if ".hip_fatbin" not in sections:  # a host-only unit
            print(f"# {os.path.basename(obj)}: no device code")
            continue
        with tempfile.TemporaryDirectory() as td:
            subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={td}/fat.bin", obj])
            subprocess.check_call([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", f"--input={td}/fat.bin",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={td}/k.co"])
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", f"{td}/k.co"], capture_output=True,
                                   text=True).stdout
            hashes = code_hashes(f"{td}/k.co") if want_hash else {}
        if len(objs) > 1:
            print(f"# {os.path.basename(obj)}")
        for b in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", b).group(1)
            if flt not in name:
                continue
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", b).group(1))
            dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            dn = dn.replace("(anonymous namespace)::", "").replace("void ", "").replace("(SearchParams)", "")
            code = f" code {hashes[name]}" if want_hash else ""
            print(f"{dn:60s} vgpr {g('vgpr_count'):4d} sgpr {g('sgpr_count'):4d} "
                  f"scratch {g('private_segment_fixed_size'):5d} lds {g('group_segment_fixed_size')}{code}")


if __name__ == "__main__":
    main()
