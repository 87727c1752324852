"""One line `symbol sha1` per device function of a HIP translation unit, sorted: the check that a host-only change left the device
code alone (same symbols, same hashes before and after).  The unit is compiled with the Makefile's flags to device assembly; each
function's text runs from `.type SYM,@function` to its `.Lfunc_end`, with the ordinals of local labels removed (they count
functions and blocks in instantiation order, which host edits move) and comment / debug-location lines dropped.  Text is hashed,
no instruction is inspected.
usage: python tools/kernel_text.py chainpartitioners.jl_amd/csrc/dp_total.hip"""
import hashlib
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chainpartitioners.jl_amd", "csrc")


def makefile_flags():
    """HIPCC and FLAGS as the Makefile spells them ($(ARCH) expanded)."""
    var = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"(\w+)\s*\??=\s*(.*)", line)
        if m:
            var[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda r: var.get(r.group(1), ""), m.group(2).strip())
    return [var["HIPCC"]] + var["FLAGS"].split()


def kernel_hashes(src):
    asm = subprocess.run(makefile_flags() + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, check=True).stdout
    out, name, body = {}, None, []
    for line in asm.split("\n"):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = line.strip()
        if t.startswith(";") or re.match(r"\.(loc|file|cfi_\w+)\b", t):
            continue
        body.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)[0-9_]+", r".L\1", line))
        if re.match(r"\.Lfunc_end\d+:", t):
            out[name] = hashlib.sha1("\n".join(body).encode()).hexdigest()
            name = None
    return out


if __name__ == "__main__":
    for sym, h in sorted(kernel_hashes(sys.argv[1]).items()):
        print(sym, h)
