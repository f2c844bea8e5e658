#!/usr/bin/env python3
"""Digest of every gfx950 kernel's instruction stream in a built libamdkge.so: the proof that a refactor only MOVED device code.

usage: kernel_isa_digest.py LIB          -> "sha256  mangled-kernel-name" per kernel, sorted by name
       kernel_isa_digest.py LIB LIB2     -> the kernels added, removed, duplicated or changed from LIB to LIB2; exit code 1 if any

Each code object of the library (one per translation unit, read with ampligraph_amd/utils/codeobj.py) is disassembled with
llvm-objdump.  What is hashed per kernel is the disassembly without its `// address: encoding` comments (absolute addresses change
when a kernel moves to another unit; branch operands are kernel-relative) and without the run of s_nop / s_code_end padding BEHIND the
kernel's last real instruction (the last kernel of a code object carries a few hundred of them; an s_nop anywhere else is hazard
padding and counts).  Digests change with the compiler: compare two builds of one toolchain, do not commit them."""
import collections, hashlib, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ampligraph_amd.utils.codeobj import _bundles   # noqa: E402


def objdump():
    return shutil.which("llvm-objdump") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def digests(lib, arch="gfx950"):
    """-> {kernel name: [sha256 of its normalised disassembly, one per code object that holds it]}"""
    out = collections.defaultdict(list)
    for triple, obj in _bundles(open(lib, "rb").read()):
        if arch not in triple or not obj:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            text = subprocess.run([objdump(), "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], check=True, capture_output=True, text=True).stdout
        name, body = None, []

        def close():
            if name is not None:
                while body and re.match(r"s_nop\b|s_code_end\b|\.\.\.$", body[-1]):   # ("...": objdump's elision of the zero fill behind them)
                    body.pop()
                out[name].append(hashlib.sha256("\n".join(body).encode()).hexdigest())

        for line in text.split("\n"):
            m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
            if m:
                close()
                name, body = m.group(1), []
            elif line.startswith("Disassembly of section"):
                close()
                name = None
            elif name is not None and line.strip():
                body.append(line.split("//")[0].strip())
        close()
    return out


def main(argv):
    if len(argv) not in (2, 3):
        print(__doc__)
        return 2
    a = digests(argv[1])
    if len(argv) == 2:
        for k in sorted(a):
            for d in a[k]:
                print(d, "", k)
        return 0
    b = digests(argv[2])
    diff = [("removed", k) for k in sorted(set(a) - set(b))] + [("added", k) for k in sorted(set(b) - set(a))]
    diff += [("duplicated", k) for k in sorted(set(a) & set(b)) if len(b[k]) > len(a[k])]
    diff += [("changed", k) for k in sorted(set(a) & set(b)) if set(a[k]) != set(b[k])]
    for what, k in diff:
        print(what, "", k)
    print("%d kernels, %d differences" % (len(b), len(diff)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
